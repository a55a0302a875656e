"""CPU: every case of tests/fas_edge_cases.py is what its name says, by index arithmetic and with the numpy statement of the FAS
stages (oracle/matlab_side.py fas_*) alone.  A case that is not would pass on the GPU while testing nothing."""
import numpy as np
import pytest

import fas_edge_cases as fc

pytestmark = [pytest.mark.filterwarnings("ignore:invalid value encountered:RuntimeWarning"),      # Inf - Inf, 0 * Inf, NaN on purpose
              pytest.mark.filterwarnings("ignore:overflow encountered:RuntimeWarning"),
              pytest.mark.filterwarnings("ignore:divide by zero encountered:RuntimeWarning")]
ms = fc.matlab_side()
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def all_minus_zero(A):
    return bool((A == 0).all() and np.signbit(A).all())


def all_plus_zero(A):
    return bool((A == 0).all() and not np.signbit(A).any())


# ---- shapes ------------------------------------------------------------------------------------------------------------------------

def test_the_groups_contain_what_the_kernels_can_get_wrong():
    S = fc.SHAPES
    assert len(set(S)) == len(S) == 11
    for axis in (0, 1):
        assert {s[axis] % 2 for s in S} == {0, 1}
    assert any(fc.last_tile(s)[0] == 1 for s in fc.TILE) and any(fc.last_tile(s)[1] == 1 for s in fc.TILE)   # a halo that is almost all clamp
    assert any(fc.last_tile(s)[0] == fc.TILE_ROWS - 1 for s in fc.TILE)                                      # one row short
    assert any(s[0] > 2 * fc.TILE_ROWS for s in fc.TILE)                                                     # a third tile row
    assert [s for s in S if fc.all_tiles_full(s)] == [(64, 4)]
    assert any(fc.half(s[0]) > fc.BLOCK_ROWS for s in fc.WG)                                                 # the output has a second block
    assert any(s[0] > fc.BLOCK_ROWS and fc.half(s[0]) <= fc.BLOCK_ROWS for s in fc.WG)                       # only the input has one
    # input and output row counts on opposite sides of 256 and of 512: a grid sized by the wrong one has a block too few or too many
    assert {(fc.row_blocks(s[0]), fc.row_blocks(fc.half(s[0]))) for s in fc.WG} == {(2, 1), (3, 2)}
    assert {s[0] for s in fc.WG} >= {2 * fc.BLOCK_ROWS - 1, 2 * fc.BLOCK_ROWS, 2 * fc.BLOCK_ROWS + 1, fc.BLOCK_ROWS + 1}
    for s in fc.MIN:
        assert min(s) == 3 and min(fc.coarse(s)) == 2
    assert [fc.channels(s) for s in S] == [1, 1, 1, 1, 1, 5, 1, 2, 1, 1, 1]
    for name, group in fc.GROUPS.items():
        picked = [s for s in fc.TAIL_SHAPES if s in group]
        assert len(picked) == 2 and {s[0] % 2 for s in picked} == {0, 1}, name


@pytest.mark.parametrize("shape", fc.SHAPES, ids=fc.tag)
def test_frames_are_noise_and_read_only(shape):
    I0, I1 = fc.frames(shape)
    C = fc.channels(shape)
    for I in (I0, I1):
        assert I.shape == shape + (C,) and I.dtype == F32 and not I.flags.writeable and I.flags.f_contiguous
        assert I.min() >= 0 and I.max() <= 255 and fc.differs_from_neighbours(I)
    assert not np.array_equal(I0, I1)
    f = fc.fields(shape)
    assert f["U"].shape == shape and f["Uc"].shape == fc.coarse(shape) and f["A"].shape == shape + (C,)
    assert np.abs(f["U"]).max() <= 2 and np.abs(f["V"]).max() <= 2 and fc.differs_from_neighbours(f["U"]) and fc.differs_from_neighbours(f["Uc"])


@pytest.mark.parametrize("shape", fc.SHAPES, ids=fc.tag)
def test_the_last_outputs_of_the_halving_stages_meet_the_clamp_where_the_size_says_so(shape):
    I0, _ = fc.frames(shape)
    restrict = lambda A: ms.fas_restrict(A, 0.5)
    for axis, n in enumerate(shape):
        assert fc.down_last_tap(n) in (n, n + 1) and fc.down_last_tap(n) > n - 1        # down: always, at either parity
        assert fc.reads_past_the_end(ms.fas_down, I0, axis)
        assert (fc.restrict_last_tap(n) > n - 1) == (n % 2 == 1)                        # restrict: at odd sizes only
        assert fc.reads_past_the_end(restrict, I0, axis) == (n % 2 == 1)
    assert ms.fas_down(I0).shape[:2] == fc.coarse(shape) == ms.fas_restrict(I0, 0.5).shape[:2]


def test_upscale_targets():
    for shape in fc.SHAPES:
        cr, cc = fc.coarse(shape)
        T = fc.upscale_targets(shape)
        assert {tuple(shape), (2 * cr, 2 * cc), (cr, cc), (cr, 2 * cc)} <= set(T) and all(r >= cr and c >= cc for r, c in T)
        assert ((200, 7) in T) == (shape in fc.MIN)
    # the large ratio: first = floor(x) - 1 is negative for many outputs
    idx, _ = ms._cubic_axis(2, 200)
    x = (np.arange(200) + 0.5) / 100.0 - 0.5
    assert int((np.floor(x) - 1 < 0).sum()) >= 100


# ---- identities the GPU test asserts against the kernels -----------------------------------------------------------------------------

@pytest.mark.parametrize("shape", fc.SHAPES, ids=fc.tag)
def test_equal_size_identities_hold_for_the_statement(shape):
    f = fc.fields(shape)
    Uc, Ur = f["Uc"], f["Ur"]
    assert np.array_equal(bits(ms.fas_upscale(Uc, 2.0, *Uc.shape)), bits((Uc * F32(2.0)).astype(F32)))
    want = (Uc + ((Uc - Ur) * F32(2.0)).astype(F32)).astype(F32)      # U = Uc here: any plane of the coarse size
    assert np.array_equal(bits(ms.fas_prolong_add(Uc, Uc, Ur, 2.0)), bits(want))


# ---- frame-sum order -------------------------------------------------------------------------------------------------------------------

def test_the_frame_sum_depends_on_its_order():
    I0, I1 = fc.order_frames()
    assert I0.shape == fc.ORDER_SHAPE + (fc.ORDER_C,) and fc.differs_from_neighbours(I0) and fc.differs_from_neighbours(I1)
    assert 2.0 < float(np.std(I1.astype(np.float64) - I0)) < 6.0
    f = fc.fields(fc.ORDER_SHAPE)
    pl = ms.fas_prepare(I0, I1, fc.B1, fc.B2)
    gd = ms.fas_gd(pl, f["U"], f["V"], fc.B1, fc.B2, fc.ORDER_C * fc.ALPHA)
    for name in ("M", "Cu", "Cv", "Du", "Dv"):
        P = pl[name] * gd
        changed = int((bits(ms._sum3(P)) != bits(fc.sum3_reversed(P))).sum())
        assert changed > 0, name
    P = pl["Du"] * gd
    assert int((bits(ms._sum3(P)) != bits(fc.sum3_reversed(P))).sum()) > P.shape[0] * P.shape[1] // 10


# ---- values --------------------------------------------------------------------------------------------------------------------------

def test_planted_pixels_are_apart_and_off_the_border():
    rows, cols = fc.VALUE_SHAPE
    P = fc.INTERIOR_PIXELS
    for k, (r, c, ch, f, v) in enumerate(P):
        assert 2 <= r <= rows - 3 and 2 <= c <= cols - 3 and ch < fc.VALUE_C
        for r2, c2 in [p[:2] for p in P[k + 1:]]:
            assert max(abs(r - r2), abs(c - c2)) >= 5
    assert [np.isnan(p[4]) for p in P] == [True, False, False] and [p[4] for p in P[1:]] == [np.inf, -np.inf]
    assert {p[:2] for p in fc.CORNER_PIXELS} == {(0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1)}
    assert {repr(float(p[4])) for p in fc.CORNER_PIXELS} == {"nan", "inf", "-inf"}
    for where, pixels in (("interior", fc.INTERIOR_PIXELS), ("corners", fc.CORNER_PIXELS)):
        I = fc.nonfinite_frames(where)
        assert sum(int((~np.isfinite(a)).sum()) for a in I) == len(pixels)
        for r, c, ch, f, v in pixels:
            assert repr(float(I[f][r, c, ch])) == repr(float(v))


@pytest.mark.parametrize("where", ["nan", "posinf", "interior"])
def test_the_statements_footprints(where):
    I0, I1 = fc.nonfinite_frames(where)
    want = fc.FOOTPRINTS[where]
    assert fc.footprint(ms.fas_gauss5(I0, ms.fas_gaussian5(1.0))) == want["gauss5"]
    pl = ms.fas_prepare(I0, I1, fc.B1, fc.B2)
    assert {k: fc.footprint(v) for k, v in pl.items()} == {k: want[k] for k in ms.FAS_PLANES}


def test_footprints_of_the_halving_stages_and_of_the_corners():
    G = ms.fas_gaussian5(1.0)
    I0, I1 = fc.nonfinite_frames("interior")
    assert fc.footprint(ms.fas_down(ms.fas_gauss5(I0, G))) == (16, 12)
    assert fc.footprint(ms.fas_down(I0)) == (9, 9) and fc.footprint(ms.fas_restrict(I0, 0.5)) == (1, 1)
    assert fc.footprint(ms.fas_gauss5(I1, G)) == (0, 25) and bool((ms.fas_gauss5(I1, G)[np.isinf(ms.fas_gauss5(I1, G))] < 0).all())
    # in the corners the clamp cuts every footprint to 3 x 3 (and repeats the pixel in it): fewer non-finite values, none lost
    C0, C1 = fc.nonfinite_frames("corners")
    assert fc.footprint(ms.fas_gauss5(C0, G)) == (9, 18) and fc.footprint(ms.fas_gauss5(C1, G)) == (0, 9)
    inner, corner = ms.fas_prepare(I0, I1, fc.B1, fc.B2), ms.fas_prepare(C0, C1, fc.B1, fc.B2)
    for name in ms.FAS_PLANES[1:]:
        bad = ~np.isfinite(corner[name])
        assert 0 < int(bad.sum()) <= 4 * 9 and int(bad.sum()) < sum(fc.footprint(inner[name]))
        assert not bad[3:-3, 3:-3].any()


def test_a_kernel_with_exact_zero_taps():
    G = ms.fas_gaussian5(0.15)
    assert int((G == 0).sum()) == 20 and int((G > 0).sum()) == 5 and G[2, 2] > 0.99
    I0, _ = fc.nonfinite_frames("posinf")
    out = ms.fas_gauss5(I0, G)
    assert fc.footprint(out) == (20, 5)      # 0 * Inf = NaN: a kernel that skips its zero taps gives 5 Inf and numbers


def test_signed_zeros():
    mz, pz = np.full(fc.VALUE_SHAPE, -0.0, F32), np.zeros(fc.coarse(fc.VALUE_SHAPE), F32)
    mzc = np.full(fc.coarse(fc.VALUE_SHAPE), -0.0, F32)
    assert all_minus_zero(ms.fas_gauss5(mz, ms.fas_gaussian5(1.0))) and all_minus_zero(ms.fas_down(mz)) and all_minus_zero(ms.fas_restrict(mz, 0.5))
    assert all_minus_zero(ms.fas_prolong_add(mz, mzc, pz, 2.0))       # -0 - +0 = -0
    assert all_plus_zero(ms.fas_prolong_add(mz, mzc, mzc, 2.0))       # -0 - -0 = +0, and -0 + +0 = +0
    assert all_plus_zero(ms.fas_upscale(mzc, 2.0, *fc.VALUE_SHAPE))   # negative cubic weights turn products positive
    assert all_minus_zero(ms.fas_upscale(mzc, 2.0, *mzc.shape))       # equal size: the weights are 0, 1, 0, 0


def test_subnormal_frames_give_subnormal_planes():
    assert fc.SUBNORMAL_SCALES == (1e-41, 1e-20)
    tiny, small = [ms.fas_prepare(*fc.subnormal_frames(s), fc.B1, fc.B2) for s in fc.SUBNORMAL_SCALES]
    for name in ms.FAS_PLANES[:8]:      # the derivatives of the 1e-41 frames are subnormal ...
        assert fc.subnormal(tiny[name]).sum() > tiny[name].size // 2, name
    for name in ms.FAS_PLANES[8:]:      # ... their products underflow to zero; those of the 1e-20 frames land subnormal
        assert (tiny[name] == 0).all() and fc.subnormal(small[name]).sum() > small[name].size // 2, name
    I0, _ = fc.subnormal_frames(1e-41)
    assert fc.subnormal(I0).sum() > I0.size // 2 and fc.subnormal(ms.fas_restrict(I0, 0.5)).sum() > 0
    assert fc.subnormal(ms.fas_down(I0)).sum() > 0 and fc.subnormal(ms.fas_gauss5(I0, ms.fas_gaussian5(1.0))).sum() > 0


def test_overflow_and_zero_divisors():
    v = fc.value_fields()
    gd_huge, gd_k0 = v["gd_huge"], v["gd_k0"]
    zero = gd_huge == 0
    assert 0 < int(zero.sum()) < zero.size and not np.signbit(gd_huge).any() and np.isfinite(gd_huge).all()   # OPnorm = Inf -> gd = +0
    assert bool((gd_k0 == np.inf).all())                                                                    # 1 / (0 * sqrt(..))
    R, A = v["R"], v["A"]
    s = (R + A).astype(F32)
    assert [bool(zero[p]) for p in v["cancel"]] == [True, True, False] and all(s[p] == 0 for p in v["cancel"]) and int((s == 0).sum()) == 3
    rhs = (s / gd_huge).astype(F32)
    assert fc.footprint(rhs) == (2, int(zero.sum()) - 2)          # 0/0 and x/0
    rhs = (s / gd_k0).astype(F32)
    assert bool((rhs == 0).all()) and 0 < int(np.signbit(rhs).sum()) < rhs.size   # x/Inf: zeros of both signs
    # products with gd == +0 are zeros of both signs: the first term of the frame sum must not meet a +0 accumulator
    P = v["planes"]["M"] * gd_huge
    assert bool(((P == 0) & np.signbit(P)).any()) and bool(((P == 0) & ~np.signbit(P)).any())
    P = v["planes"]["M"] * gd_k0
    assert bool(np.isinf(P).all()) and np.isnan(ms._sum3(P)).any()           # +Inf + -Inf over the frames


def test_one_nan_in_the_flow():
    v = fc.value_fields()
    r, c = v["nan_at"]
    assert int(np.isnan(v["Unan"]).sum()) == 1 and np.isnan(v["Unan"][r, c])
    gd = ms.fas_gd(v["planes"], v["Unan"], v["V"], fc.B1, fc.B2, fc.ALPHA)
    bad = np.isnan(gd)
    assert bad[r, c, :].all() and int(bad.sum()) == fc.VALUE_C                 # the per-frame outputs: at that pixel only
    zero = np.zeros(fc.VALUE_SHAPE, F32)
    for w in ms.op_diff_weights(v["Unan"], v["V"], zero, zero):                # the weights: the pixel and its neighbours
        bad = np.isnan(w)
        assert bad[r, c] and int(bad.sum()) > 1 and not bad[:r - 2].any() and not bad[r + 3:].any() and not bad[:, :c - 2].any() and not bad[:, c + 3:].any()


def test_the_driver_case_has_a_seam_at_every_transfer():
    rows, cols = fc.SEAM_DRIVER_SHAPE
    P0, _ = ms.fas_pyramid(*fc.frames(fc.SEAM_DRIVER_SHAPE, fc.SEAM_DRIVER_C))
    assert [p.shape[:2] for p in P0] == [(259, 23), (130, 12), (65, 6)]
    assert rows > fc.BLOCK_ROWS and fc.half(rows) <= fc.BLOCK_ROWS
