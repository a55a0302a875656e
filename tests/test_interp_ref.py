"""CPU: the restatement of the frame interpolation (interp_ref.py) pinned against closed forms -- zero flow, an integer translation,
the contraction onto one pixel, every row of the blend's table -- and then its quality on the 96 x 128 scene of interp_cases.py
(a textured square moving 6 px over a static textured background, true flows, the middle frame rendered analytically).

Measured with the oracle's solver (printed below), RMS error against the true middle frame over the valid pixels, grey levels of a
0..1 image: 0.0691 for the plain average (I0 + I1) / 2, 0.0165 for the chain without the backward flow, 0.0006 with it."""
import numpy as np
import pytest

import interp_cases as ic
import interp_ref as ir
import problems as pb

F32, F64 = np.float32, np.float64


def same(got, want, what):
    assert pb.bit_equal(got, want), "%s: %s" % (what, pb.describe_mismatch(got, want))


def test_zero_flow():
    for shape in ((3, 3), (37, 53)):
        Uf, Vf, I0, I1 = ic.field(shape, "zero")
        for t in (ic.T_LOW, ic.T_HALF, ic.T_HIGH):
            Ut, Vt, cost, winner = ir.flow_splat(Uf, Vf, t, I0, I1)
            assert Ut.tobytes() == Uf.tobytes() and Vt.tobytes() == Vf.tobytes()
            assert np.array_equal(winner, np.arange(Uf.size).reshape(shape, order="F"))
            want_cost = np.abs(I0.astype(F64) - I1.astype(F64))
            total = np.zeros(shape)
            for ch in range(I0.shape[2]):
                total = total + want_cost[:, :, ch]
            same(cost, total.astype(F32), "cost at zero flow")
            It, src = ir.interp_blend(I0, I1, Ut, Vt, t)
            same(It, ((1.0 - t) * I0.astype(F64) + t * I1.astype(F64)).astype(F32), "zero-flow blend")
            assert (src == 3).all()


def test_integer_shift_moves_the_frame_by_t_d(oracle):
    """d = (2, -2), t = 0.5, I1 = I0 moved by d: inside the band the frame at t is I0 moved by (1, -1), bit for bit (both samples
    are the same pixel of I0 with weight 1, and 0.5 a + 0.5 a == a)."""
    shape = (37, 53)
    Uf, Vf, I0, _ = ic.field(shape, "shift_even")
    u, v = (int(x) for x in ic.SHIFT_EVEN)
    I1 = np.array(I0)
    I1[:-2, u:, :] = I0[2:, :-u, :]            # I1(x, y) = I0(x - u, y - v), v = -2
    assert v == -2
    It, Ut, Vt, src = ir.flow_interpolate(oracle, I0, I1, Uf, Vf, t=0.5)
    band = (slice(4, -4), slice(4, -4))
    want = np.array(I0)
    want[:-1, 1:, :] = I0[1:, :-1, :]          # It(x, y) = I0(x - 1, y + 1)
    assert It[band].tobytes() == want[band].tobytes()
    assert (src[band] == 3).all()
    assert (Ut[band] == u).all() and (Vt[band] == v).all()
    # a constant flow leaves only the border band empty, and the filling keeps what was splatted
    sUt, _, _, _ = ir.flow_splat(Uf, Vf, 0.5, I0, I1)
    assert np.isnan(sUt[:, 0]).all() and np.isnan(sUt[-1, :]).all() and not np.isnan(sUt[:-1, 1:]).any()
    # q0 = (x - 1, y + 1) and q1 = (x + 1, y - 1) both leave the frame at two corners (the filled border is 2, -2 only nearly)
    assert np.array_equal(np.isnan(It[:, :, 0]), src == 0) and src[0, 0] == 0 and src[-1, -1] == 0 and (src == 0).sum() < 6


def test_contraction_goes_to_the_lowest_index_or_the_lowest_cost():
    for shape in ((3, 3), (5, 90), (37, 53)):
        Uf, Vf, I0, I1 = ic.field(shape, "contract")
        cy, cx = (shape[0] + 1) // 2 - 1, (shape[1] + 1) // 2 - 1
        Ut, Vt, cost, winner = ir.flow_splat(Uf, Vf, 0.5)
        assert (winner >= 0).sum() == 1 and winner[cy, cx] == 0, "equal costs: the first pixel in memory"
        assert Ut[cy, cx] == Uf[0, 0] and Vt[cy, cx] == Vf[0, 0] and cost[cy, cx] == 0
        Ut, Vt, cost, winner = ir.flow_splat(Uf, Vf, 0.5, I0, I1)
        c = ir.splat_costs(Uf, Vf, I0, I1).reshape(-1, order="F")
        assert (winner >= 0).sum() == 1 and winner[cy, cx] == int(np.argmin(c)), "argmin takes the first of equal minima as well"
        assert cost[cy, cx] == c.min()
        assert np.isnan(Ut).sum() == Ut.size - 1


def test_costs_decide_where_two_layers_cross():
    Uf, Vf, I0, I1 = ic.field((37, 53), "layers")
    Ut, Vt, cost, winner = ir.flow_splat(Uf, Vf, 0.5, I0, I1)
    half = 53 // 2
    both = slice(half - 1, half + 1)          # columns reached from both sides: 1-based half, half + 1
    assert (Ut[:, both] == 2.0).all(), "frame 1 agrees with the layer moving right"
    plain = ir.flow_splat(Uf, Vf, 0.5)[0]
    assert (plain[:, both] == 2.0).all(), "without costs the lower index wins, here the same layer"
    flipped = ir.flow_splat(Uf, Vf, 0.5, I1, I0)[0]    # costs of the wrong pairing
    assert not (flipped[:, both] == 2.0).all()


def test_nonfinite_sources_and_signed_zeros():
    Uf, Vf, I0, I1 = ic.field((37, 53), "nonfinite")
    Ut, Vt, cost, winner = ir.flow_splat(Uf, Vf, 0.5, I0, I1)
    src = np.isfinite(Uf) & np.isfinite(Vf)
    won = winner[winner >= 0]
    assert src.reshape(-1, order="F")[won].all() and not src.all()
    assert np.isinf(cost[winner >= 0]).any(), "a source with a NaN sample still splats, at cost +Inf"
    assert np.array_equal(np.isnan(Ut), winner < 0) and np.array_equal(np.isnan(cost), winner < 0)
    Uf, Vf, I0, I1 = ic.field((37, 53), "neg_zero")
    Ut, Vt, _, winner = ir.flow_splat(Uf, Vf, 0.5, I0, I1)
    hit = winner >= 0
    assert Ut[hit].tobytes() == Uf.reshape(-1, order="F")[winner[hit]].tobytes() and np.signbit(Ut[hit]).any()
    Uf, Vf, I0, I1 = ic.field((37, 53), "all_nonfinite")
    assert (ir.flow_splat(Uf, Vf, 0.5, I0, I1)[3] < 0).all()


def test_an_expansion_leaves_holes():
    Uf, Vf, I0, I1 = ic.field((37, 53), "expand")
    for t in (0.25, 0.5):
        hole = ir.flow_splat(Uf, Vf, t, I0, I1)[3] < 0
        assert 0.2 < hole.mean() < 0.95 and not hole[18, 26], "the centre stays where it is"


def test_landings_on_the_last_line_and_one_ulp_outside():
    Uf, Vf, _, _ = ic.field((5, 90), "edges")
    Ut, Vt, _, winner = ir.flow_splat(Uf, Vf, 0.5)
    # only the first and last row / column can be reached, and the four corners take every source that stays inside
    inner = winner[1:-1, 1:-1]
    assert (inner < 0).all() and (winner[0, 0] >= 0) and (winner[-1, -1] >= 0)
    i, j = np.meshgrid(np.arange(5), np.arange(90), indexing="ij")
    inside = ((i + j) % 4 < 2) & ((i + 2 * j) % 4 < 2)     # neither displacement one ulp beyond
    assert (winner >= 0).sum() == len({((i[a, b] + 2 * j[a, b]) % 4, (i[a, b] + j[a, b]) % 4) for a, b in zip(*np.nonzero(inside))})


def test_every_row_of_the_table():
    shape = (5, 9)
    rng = np.random.default_rng(3)
    I0, I1 = rng.random(shape).astype(F32), rng.random(shape).astype(F32)
    U = np.full(shape, 4.0, F32)
    V = np.zeros(shape, F32)
    U[2, 4] = np.nan
    V[3, 4] = np.inf
    It, src = ir.interp_blend(I0, I1, U, V, 0.5)
    want = np.empty(shape, F32)
    want[:, :2], want[:, 2:7], want[:, 7:] = 2, 3, 1       # q0 = x - 2 leaves on the left, q1 = x + 2 on the right
    want[2, 4] = want[3, 4] = 0
    assert np.array_equal(src, want)
    assert np.isnan(It[2, 4]) and np.isnan(It[3, 4])
    assert It[:, :2].tobytes() == I1[:, 2:4].tobytes() and It[:, 7:].tobytes() == I0[:, 5:7].tobytes()
    same(It[0, 2:7], (0.5 * I0[0, 0:5].astype(F64) + 0.5 * I1[0, 4:9].astype(F64)).astype(F32), "both")
    far = np.full(shape, 40.0, F32)
    assert (ir.interp_blend(I0, I1, far, np.zeros(shape, F32), 0.5)[1] == 0).all()
    # the masks, at zero flow: the sample that fails its own check is the one shown
    Z = np.zeros(shape, F32)
    M0 = np.tile(np.array([1, 1, 0, 0, 1, 1, 0, 0, 1], F32), (5, 1))
    M1 = np.tile(np.array([1, 0, 1, 0, 1, 0, 1, 0, 1], F32), (5, 1))
    It, src = ir.interp_blend(I0, I1, Z, Z, 0.25, M0, M1)
    assert np.array_equal(src[0], np.array([3, 2, 1, 3, 3, 2, 1, 3, 3], F32))
    assert It[:, 1].tobytes() == I1[:, 1].tobytes() and It[:, 2].tobytes() == I0[:, 2].tobytes()
    same(It[:, 3], (0.75 * I0[:, 3].astype(F64) + 0.25 * I1[:, 3].astype(F64)).astype(F32), "both fail: blended")
    # the nearest pixel of a sample half way between two is the next one; beyond the last it is the last
    Uh = np.full(shape, 2.0, F32)                          # q0 = x - 0.5, q1 = x + 1.5 at t = 0.25
    M0 = np.ones(shape, F32)
    M1 = np.ones(shape, F32)
    M0[:, 3] = 0                                           # nearest(q0) of x = 4 (1-based) is floor(3.5 + 0.5) = 4, i.e. column index 3
    _, src = ir.interp_blend(I0, I1, Uh, Z, 0.25, M0, M1)
    assert (src[:, 3] == 1).all() and (src[:, 2] == 3).all() and (src[:, 4] == 3).all()


@pytest.fixture(scope="module")
def scene_runs(oracle):
    I0, I1, Imid, Uf, Vf, Ub, Vb, valid = ic.scene()
    return dict(forward=ir.flow_interpolate(oracle, I0, I1, Uf, Vf, t=0.5), both=ir.flow_interpolate(oracle, I0, I1, Uf, Vf, Ub, Vb, t=0.5))


def test_quality_on_the_scene(scene_runs):
    I0, I1, Imid, Uf, Vf, Ub, Vb, valid = ic.scene()
    a = ic.rms(((I0.astype(F64) + I1.astype(F64)) / 2).astype(F32), Imid, valid)
    b = ic.rms(scene_runs["forward"][0], Imid, valid)
    c = ic.rms(scene_runs["both"][0], Imid, valid)
    print("scene: RMS against the true middle frame: average of the frames %.4f, chain without backward flow %.4f, with it %.4f" % (a, b, c))
    src = scene_runs["both"][3]
    print("scene: source plane with the backward flow: %r" % {int(k): int((src == k).sum()) for k in np.unique(src)})
    assert b < a
    assert c <= b
    for run in scene_runs.values():
        assert np.isfinite(run[0]).all() and np.isfinite(run[1]).all() and np.isfinite(run[2]).all()
    assert set(np.unique(scene_runs["forward"][3])) == {3.0}
    assert {1.0, 2.0, 3.0} <= set(np.unique(src))


def test_a_field_without_a_source_is_the_zero_flow_blend(oracle):
    """What pdeip_tv_inpaint4 makes of an all-hole plane: the mean of no known pixel is 0, and diffusion keeps it 0."""
    Uf, Vf, I0, I1 = ic.field((37, 53), "all_nonfinite")
    It, Ut, Vt, src = ir.flow_interpolate(oracle, I0, I1, Uf, Vf, t=0.25)
    assert (Ut.view(np.uint32) == 0).all() and (Vt.view(np.uint32) == 0).all()
    same(It, (0.75 * I0.astype(F64) + 0.25 * I1.astype(F64)).astype(F32), "all holes")
    assert (src == 3).all()
