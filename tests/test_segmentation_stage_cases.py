"""CPU: every case of tests/segmentation_stage_cases.py is what its name says, and the order model of the library's sums
(segmentation_ref.variance_in_order) is variance() in everything but the order.

The GPU tests (test_gpu_segmentation_stages.py) only consume the cases; what a case contains -- the tile, wave and batch seam a
plane stands at, the edge elements, the values at the edge of the range, where the restatement's P is subnormal or zero -- is proved
here, against numpy alone.  So is the comparison rule the GPU tests use at the range cases: with exp, expm1 and log each a whole
ulp off, no NaN or Inf of DATA moves and no DATA moves further than the adjacent float."""
import numpy as np
import pytest

import segmentation_cases as sc
import segmentation_ref as sr
import segmentation_stage_cases as ssc

F32 = np.float32
TINY = np.finfo(np.float64).tiny
STRATEGIES = sorted(sr.STRATEGY)


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def same_cov(a, b):
    """Bit for bit; a NaN equals any NaN."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(_bits(a)[~np.isnan(a)], _bits(b)[~np.isnan(b)]))


# ---- the seam planes ---------------------------------------------------------------------------------------------------------------

def test_the_seam_planes_stand_where_the_table_says():
    npix = {s: s[0] * s[1] for s in ssc.SEAM_PLANES}
    assert sorted(npix.values()) == [4, 63, 64, 65, 255, 256, 258, 3840, 4095, 4096, 4097, 7936, 8192, 8193, 65536, 65631]
    for shape, (tiles, last_tile, last_wave) in ssc.SEAM_PLANES.items():
        n = npix[shape]
        assert min(shape) >= 2
        assert tiles == -(-n // ssc.TILE) and last_tile == n - (tiles - 1) * ssc.TILE and 1 <= last_tile <= ssc.TILE
        assert last_wave == (last_tile - 1) % ssc.WAVE + 1
        assert ssc.edges(shape) == ((tiles - 1) * ssc.TILE, n - 1)
    tiles = sorted(t for t, _, _ in ssc.SEAM_PLANES.values())
    assert tiles == [1] * 6 + [2, 15, 16, 16, 17, 31, 32, 33, 256, 257]
    # the batch of 16: trips and tail of k_seg_variance_final's two loops
    assert sorted({(t // ssc.AHEAD, t % ssc.AHEAD) for t in tiles if t >= 15}) == [(0, 15), (1, 0), (1, 1), (1, 15), (2, 0), (2, 1), (16, 0), (16, 1)]
    assert [t > 256 for t in tiles] == [False] * 15 + [True]  # k_seg_sizes_final's second trip
    assert all(n > 65000 for s, n in npix.items() if s in ssc.BIG_PLANES) and all(ssc.seam_s(s) == (1, 3) for s in ssc.BIG_PLANES)
    assert {S for _, S in ssc.MANY_CASES} == {255, 256, 257} and {s for s, _ in ssc.MANY_CASES} == {(5, 13), (17, 241)}
    assert not any(s == (17, 241) and S > 17 for s, S in ssc.DATA_CASES) and sum(S > 17 for _, S in ssc.DATA_CASES) == 3
    assert max(s[0] * s[1] * S for s, S in ssc.SEAM_CASES + ssc.MANY_CASES) == 17 * 241 * 257


@pytest.mark.parametrize("case", ssc.SEAM_CASES + ssc.MANY_CASES, ids=ssc.case_id)
def test_seam_case_follows_the_recipe_and_marks_its_edges(case):
    shape, S = case
    PHI, dist, DH = ssc.seam_case(shape, S)
    assert PHI.shape == dist.shape == DH.shape == shape + (S,) and PHI.dtype == dist.dtype == DH.dtype == F32
    assert not PHI.flags.writeable and PHI.flags.f_contiguous
    assert np.isnan(PHI).sum() == 1 and (np.signbit(PHI) & (PHI == 0)).any() and (~np.signbit(PHI) & (PHI == 0)).any()
    assert (dist > 100).any() and (dist < 100).any() and not np.isnan(dist).any()
    if shape != (2, 2):
        assert (DH > F32(0.02)).any() and (DH < F32(0.02)).any()
    first, last = ssc.edges(shape)
    for p in {first, last}:
        i, j = ssc.at(shape, p)
        assert (PHI[i, j, :] >= 0).all()
        assert [(dist[:, :, s] == dist[i, j, s]).sum() for s in range(S)] == [1] * S  # a dist no other pixel of the segment has
    # an edge element dropped shows in n and in the sum (cov is far above the floor)
    cov, n = ssc.want_variance(shape, S, 1e-3, np.inf)
    for p in {first, last}:
        i, j = ssc.at(shape, p)
        less = PHI.copy()
        less[i, j, :] = -1
        c2, n2 = sr.variance_in_order(less, dist, 1e-3, np.inf)
        assert (n2 == n - 1).all() and (c2 != cov).all()


# ---- the order model ---------------------------------------------------------------------------------------------------------------

def _model_against_cumsum(PHI, dist, what):
    differ = 0
    for cap in (np.inf, 100.0):
        for minCOV in (1e-3, 1e3):
            cov, n = sr.variance_in_order(PHI, dist, minCOV, cap)
            with np.errstate(invalid="ignore"):  # cumsum over +Inf and -Inf
                want, wn = sr.variance(PHI, dist, minCOV, cap)
            assert cov.dtype == np.float64 and np.array_equal(n, wn), what
            assert np.array_equal(np.isnan(cov), np.isnan(want)) and np.array_equal(np.isinf(cov), np.isinf(want)), what
            fin = np.isfinite(want)
            assert np.array_equal(np.sign(cov[~fin & ~np.isnan(want)]), np.sign(want[~fin & ~np.isnan(want)])), what
            assert (np.abs(cov[fin] - want[fin]) <= 2.0 * wn[fin] * 2.0 ** -53 * np.abs(want[fin])).all(), what
            differ += int((_bits(cov)[fin] != _bits(want)[fin]).sum())
    return differ


@pytest.mark.parametrize("case", ssc.SEAM_CASES + ssc.MANY_CASES, ids=ssc.case_id)
def test_the_order_model_is_variance_in_another_order(case):
    """Equal n, equal NaN and Inf, cov within the tolerance the suite has used so far -- and not in the same bits where the plane
    is large enough for the order to matter: there the bit test says what the tolerance does not."""
    shape, S = case
    PHI, dist, _ = ssc.seam_case(shape, S)
    _model_against_cumsum(PHI, dist, ssc.case_id(case))
    if ssc.SEAM_PLANES[shape][0] >= 15 and S == 17:
        cov, _ = sr.variance_in_order(PHI, dist, 1e-3, np.inf)
        want, _ = sr.variance(PHI, dist, 1e-3, np.inf)
        assert (_bits(cov) != _bits(want)).any()


@pytest.mark.parametrize("shape", sc.STAGE_SHAPES)
def test_the_order_model_on_the_habitual_stage_planes(shape):
    PHI, dist, _ = sc.stage_case(shape, 17)
    assert _model_against_cumsum(PHI, dist, str(shape)) > 0
    PHI, dist, _ = sc.stage_case(shape, 17, nan_dist=True)
    _model_against_cumsum(PHI, dist, str(shape) + " with a NaN dist")


@pytest.mark.parametrize("shape", ssc.SEAM_PLANES, ids=lambda s: "%dx%d" % s)
def test_the_order_model_depends_neither_on_S_nor_on_s(shape):
    """Step 2c: 'a fixed order that depends neither on S nor on s'."""
    P1, d1, _ = ssc.seam_case(shape, 1)
    S = 3 if shape in ssc.BIG_PLANES else 17
    PHI, dist, _ = (a.copy() for a in ssc.seam_case(shape, S))
    for cap in (np.inf, 100.0):
        one, n1 = sr.variance_in_order(P1, d1, 1e-3, cap)
        for s in (0, S // 2, S - 1):
            PHI[:, :, s], dist[:, :, s] = P1[:, :, 0], d1[:, :, 0]
            cov, n = sr.variance_in_order(PHI, dist, 1e-3, cap)
            assert n[s] == n1[0] and _bits(cov)[s] == _bits(one)[0]


@pytest.mark.parametrize("shape", ssc.SEAM_PLANES, ids=lambda s: "%dx%d" % s)
def test_variance_edge_segments(shape):
    PHI, dist = ssc.variance_edge_case(shape)
    assert PHI.shape == shape + (4,) and ssc.VARIANCE_EDGES == ("empty", "plus_inf", "minus_inf", "both_inf")
    inside = sr.mask(PHI)
    assert not inside[:, :, 0].any()
    assert [int((np.isposinf(dist[:, :, s]) & inside[:, :, s]).sum()) for s in range(4)] == [0, 1, 0, 1]
    assert [int((np.isneginf(dist[:, :, s]) & inside[:, :, s]).sum()) for s in range(4)] == [0, 0, 1, 1]
    for fn in (sr.variance_in_order, sr.variance):
        for minCOV in (1e-3, 1e3):
            with np.errstate(invalid="ignore"):  # cumsum over +Inf and -Inf
                cov, n = fn(PHI, dist, minCOV, np.inf)
            assert n[0] == 0 and np.isnan(cov[0]) and cov[1] == np.inf and cov[2] == minCOV and np.isnan(cov[3])
            cov, n = fn(PHI, dist, minCOV, 100.0)
            assert n[0] == 0 and np.isnan(cov[0]) and np.isfinite(cov[1]) and cov[2] == minCOV and cov[3] == minCOV
    _model_against_cumsum(PHI, dist, "edges %s" % (shape,))


@pytest.mark.parametrize("case", ssc.SEAM_CASES + ssc.MANY_CASES, ids=ssc.case_id)
def test_label_case(case):
    shape, S = case
    PHI = ssc.label_case(shape, S)
    want = sr.label(PHI)
    first, last = ssc.edges(shape)
    assert want[ssc.at(shape, last)] == S and (PHI[ssc.at(shape, last)] > 0).sum() == 1
    over = first if first != last else first - ssc.TILE
    if S >= 2 and over >= 0:
        assert want[ssc.at(shape, over)] == 0 and (PHI[ssc.at(shape, over)] > 0).sum() == 2
    assert np.isnan(PHI).any() and (PHI == 0).any()
    if shape[0] * shape[1] >= 63:
        assert len(np.unique(want)) >= min(S, 8) and (want == 0).any()


# ---- the range cases ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ssc.RANGE_PLANES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("S", ssc.STAGE_S)
def test_range_case_holds_every_listed_value_in_every_segment(shape, S):
    PHI, dist, DH, together, alone = ssc.range_case(shape, S)
    listed = [float(v) for v in ssc.RANGE_DIST]
    assert listed[:2] == [0.0, 0.0] and np.signbit(ssc.RANGE_DIST[1]) and listed[5:9] == [700.0, 1400.0, 1480.0, 1500.0]
    assert 0 < listed[2] < listed[3] < np.finfo(F32).tiny and 3.39e38 < listed[9] < np.inf and listed[10:] == [np.inf, -1.0, -np.inf]
    assert len(set(together.tolist()) | set(alone.ravel().tolist())) == len(listed) * (S + 1)
    for k, v in enumerate(ssc.RANGE_DIST):
        i, j = ssc.at(shape, together[k])
        assert ssc.same_bits(dist[i, j, :], v).all()
        assert np.array_equal(PHI[i, j, :] >= 0, np.arange(S) % 2 == 0)
        for s in range(S):
            i, j = ssc.at(shape, alone[k, s])
            assert ssc.same_bits(dist[i, j, s], v)
    # the strips: no segment inside, DH at and next to 0.02f
    assert not sr.mask(PHI[:, :3, :]).any()
    below, exact, above = (DH[:, ssc.STRIP[k], :] for k in ("below", "exact", "above"))
    assert (exact == F32(0.02)).all() and (below < F32(0.02)).all() and (above > F32(0.02)).all()
    assert (np.nextafter(below, F32(1)) == exact).all() and (np.nextafter(above, F32(-1)) == exact).all()
    assert np.isnan(PHI).any() and (np.signbit(PHI) & (PHI == 0)).any()


def test_range_covs():
    for S in ssc.STAGE_S:
        covs = ssc.range_covs(S)
        assert (covs["ones"] == 1).all()
        edge = [c[c != 1] for k, c in covs.items() if k != "ones"]
        if S == 17:
            assert len(edge) == 1 and same_cov(edge[0], ssc.COV_EDGES)
        else:
            assert len(edge) == 8 and all(e.size == 1 for e in edge) and same_cov(np.concatenate(edge), ssc.COV_EDGES)
    assert ssc.COV_EDGES[0] == np.nextafter(0.0, 1.0) and 0 < ssc.COV_EDGES[1] < 1e-299
    assert len(ssc.RANGE_CASES) == 2 * (3 * 9 + 2)


@pytest.mark.parametrize("shape", ssc.RANGE_PLANES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("S", ssc.STAGE_S)
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_range_case_reaches_the_edges_of_float64(shape, S, strategy):
    """With cov = 1 the restatement's P is a float64 subnormal at some pixel and exactly 0 at another, +Inf at a third; DATA holds
    +Inf, and -Inf where there is a competitor; at S = 17 at least three quarters of DATA stay finite, whatever the cov."""
    w = ssc.want_range_data(shape, S, "ones", sr.STRATEGY[strategy])
    P, DATA = w["P"], w["DATA"]
    assert ((P > 0) & (P < TINY)).any() and (P == 0).any() and np.isposinf(P).any() and np.isnan(DATA).any() == (S > 1 or strategy == "inverse")
    assert np.isposinf(DATA).any() == (S > 1 or strategy != "inverse")
    assert np.isneginf(DATA).any() == (S > 1)
    for name in ssc.range_covs(S):
        DATA = ssc.want_range_data(shape, S, name, sr.STRATEGY[strategy])["DATA"]
        share = np.isfinite(DATA).mean()
        print("%s S=%d %s cov %s: %.1f %% of DATA finite" % (shape, S, strategy, name, 100 * share))
        if S == 17:
            assert share >= 0.75


@pytest.mark.parametrize("shape", ssc.RANGE_PLANES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("S", (2, 3, 17))
def test_greedy_changes_the_competitor_on_one_side_of_the_threshold_only(shape, S):
    PHI, dist, DH, _, _ = ssc.range_case(shape, S)
    greedy = ssc.want_range_data(shape, S, "ones", sr.GREEDY)["WC"]
    surface = ssc.want_range_data(shape, S, "ones", sr.SURFACE)["WC"]
    assert (surface[:, :3, :] > 0).all()
    assert (greedy[:, ssc.STRIP["above"], :] == 0).all()
    for k in ("below", "exact"):
        assert np.array_equal(greedy[:, ssc.STRIP[k], :], surface[:, ssc.STRIP[k], :])
    assert not (DH[:, 3:, :] == F32(0.02)).any()


# ---- the comparison rule is robust at these inputs ------------------------------------------------------------------------------------

class _OffByAnUlp:
    """numpy with exp, expm1 and log moved one ulp up (+1) or down (-1) wherever their result is finite and not zero: a pessimistic
    stand-in for a second maths library."""

    def __init__(self, move):
        self.move = move

    def __getattr__(self, name):
        fn = getattr(np, name)
        if self.move.get(name, 0) == 0:
            return fn
        to = np.inf * self.move[name]

        def moved(x):
            y = fn(x)
            return np.where(np.isfinite(y) & (y != 0), np.nextafter(y, to), y)

        return moved


MOVES = [dict(exp=d, expm1=d, log=d) for d in (1, -1)] + [{f: d} for f in ("exp", "expm1", "log") for d in (1, -1)] + [dict(exp=1, expm1=-1, log=-1), dict(exp=-1, expm1=1, log=1)]


@pytest.mark.parametrize("case", ssc.RANGE_CASES, ids=ssc.range_id)
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_an_ulp_in_the_maths_library_moves_no_pattern_and_no_data_by_more_than_a_float(monkeypatch, case, strategy):
    """What licenses the project's rule (NaN and Inf patterns equal, DATA equal or the adjacent float) on the GPU at these inputs: it
    holds between the float64 restatement and itself with exp, expm1 and log a whole ulp off, up or down, together or alone.  (The
    long-double recomputation is no yardstick here: where P and WC are far below eps, DATA ~ (P - WC)/eps carries the float64
    rounding of P + eps, which the contract defines and a wider format does not reproduce.)"""
    shape, S, name = case
    PHI, dist, DH, _, _ = ssc.range_case(shape, S)
    cov = ssc.range_covs(S)[name]
    want = ssc.want_range_data(shape, S, name, sr.STRATEGY[strategy])["DATA"]
    fin = np.isfinite(want)
    worst = 0.0
    for move in MOVES:
        with monkeypatch.context() as m:
            m.setattr(sr, "np", _OffByAnUlp(move))
            got = sr.data_term(dist, PHI, DH, cov, sr.STRATEGY[strategy])["DATA"]
        assert got.dtype == F32
        assert np.array_equal(np.isnan(got), np.isnan(want)), move
        assert np.array_equal(np.isposinf(got), np.isposinf(want)) and np.array_equal(np.isneginf(got), np.isneginf(want)), move
        differ = got[fin] != want[fin]
        assert (np.nextafter(want[fin][differ], got[fin][differ]) == got[fin][differ]).all(), move
        worst = max(worst, differ.mean() if differ.size else 0.0)
    print("%s %s: at most %.3g %% of the finite DATA moved to the adjacent float" % (ssc.range_id(case), strategy, 100 * worst))
    assert worst <= 1e-3  # the GPU rule's share is within reach of any library that is an ulp off: no float32 ties built into the case
