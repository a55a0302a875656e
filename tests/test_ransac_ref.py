"""CPU: the restatement of SurfaceEquation (ransac_ref.py) on its own, the conditions on the inputs the GPU tests use
(ransac_cases.py), and every refusal of the C-ABI and of the MEX stub that fires before any HIP call."""
import ctypes

import numpy as np
import pytest

import ransac_cases as rc
import ransac_ref as ref
from test_capi_symbols import declared_symbols
from test_mex_stubs import call

F32 = np.float32
ENTRIES = ["pdeip_surface_equation", "pdeip_surface_equation_dev", "pdeip_surface_fit_masked_dev"]

# ---- the QR is a least-squares solve ------------------------------------------------------------------------------------------
# max |x_qr - x_lstsq| / (cond(A) * 2^-52 * max |x_lstsq|) over 200 seeded systems per order, coordinates from a 480 x 640 grid with
# the samples at least 8 px apart, B uniform in 0..64; numpy.linalg.lstsq (LAPACK gelsd) in float64 on the same widened samples.
#   measured (numpy 2.x, OpenBLAS):  order 1: 0.233   order 2: 0.00129   (absolute: 5.5e-14 and 8.5e-13 relative to max |x|)
#   bound = 8 x measured, for other LAPACK builds:
QR_MEASURED = {1: 0.233, 2: 0.00129}
QR_BOUND = {1: 8 * 0.233, 2: 8 * 0.00129}


def _spread_samples(rng, n):
    while True:
        X = rng.integers(1, 641, n)
        Y = rng.integers(1, 481, n)
        d = np.hypot(X[:, None] - X[None, :], Y[:, None] - Y[None, :]) + np.eye(n) * 1e9
        if d.min() >= 8:
            return X, Y


@pytest.mark.parametrize("order", [1, 2])
def test_qr_is_a_least_squares_solve(order):
    rng = np.random.default_rng(1234 + order)
    n = 4 if order == 1 else 7
    worst = 0.0
    for _ in range(200):
        X, Y = _spread_samples(rng, n)
        A = ref.design(X, Y, order)
        B = rng.uniform(0, 64, n).astype(F32)
        want = np.linalg.lstsq(A.astype(np.float64), B.astype(np.float64), rcond=None)[0]
        x, singular = ref.fit64(A, B)
        assert not singular
        cond = np.linalg.cond(A.astype(np.float64))
        worst = max(worst, np.abs(np.array(x) - want).max() / (cond * 2.0 ** -52 * np.abs(want).max()))
        m, _ = ref.fit(A, B)
        assert np.array_equal(m, np.array(x).astype(F32))
    print("order %d: max error / (cond * 2^-52 * max|x|) = %.3g (bound %.3g)" % (order, worst, QR_BOUND[order]))
    assert worst <= QR_BOUND[order]


def test_fit_many_is_fit_lane_by_lane():
    """The vectorised form the other tests use against the plain loops over Python floats: the same bits, singular systems and a
    NaN sample included."""
    for order in (1, 2):
        A, B = rc.surface_points(7 + order, 500, order)
        B = B.copy()
        B[3] = np.nan
        n = A.shape[1] + 1
        sets = ref.sample_sets(9, 40, n, 500)
        sets[5, :] = 77   # n identical rows
        sets[6, 0] = 3    # a NaN right-hand side
        sets[7, :2] = 11  # one duplicate
        M, sing = ref.fit_many(A[sets], B[sets])
        for h in range(40):
            m, s = ref.fit(A[sets[h]], B[sets[h]])
            assert s == sing[h], h
            assert np.array_equal(np.isnan(m), np.isnan(M[h])) and np.array_equal(m[~np.isnan(m)].view(np.uint32), M[h][~np.isnan(m)].view(np.uint32)), h
        assert sing[5] and not M[5].any() and np.isnan(M[6]).all()


def test_exact_plane_is_recovered():
    X = np.array([3, 200, 90, 610])
    Y = np.array([5, 17, 400, 333])
    A = ref.design(X, Y, 1)
    B = (0.25 * X - 0.5 * Y + 3).astype(F32)
    m, singular = ref.fit(A, B)
    assert not singular and np.allclose(m, [0.25, -0.5, 3], rtol=1e-6, atol=1e-6)
    assert ref.errors(A, B, m).max() < 1e-6
    assert ref.fit(A[[0, 0, 0, 0]], B[[0, 0, 0, 0]])[1]  # four times one row: singular


# ---- sample_sets ---------------------------------------------------------------------------------------------------------------

def test_sample_sets_are_reproducible_and_in_range():
    assert ref.splitmix64(0) == 0xE220A8397B1DCDAF  # the first output of SplitMix64 seeded with 0
    for ndata in (1, 4, 65, 20011, 307200):
        a = ref.sample_sets(12345, 50, 7, ndata)
        assert a.dtype == np.uint32 and a.shape == (50, 7)
        assert np.array_equal(a, ref.sample_sets(12345, 50, 7, ndata))
        assert a.max() < ndata
    assert not np.array_equal(ref.sample_sets(1, 50, 4, 20011), ref.sample_sets(2, 50, 4, 20011))
    a = ref.sample_sets(2 ** 64 - 3, 4, 4, 1000)  # seed + i*n + k wraps
    assert np.array_equal(a.ravel()[3:], ref.sample_sets(0, 4, 4, 1000).ravel()[:13])
    big = ref.sample_sets(7, 2000, 4, 5)
    assert set(np.unique(big)) == {0, 1, 2, 3, 4}


# ---- the selection rules on hand-made score lists --------------------------------------------------------------------------------

def test_licit_path_is_strict():
    w, _ = ref.select([10, 10, 10], [2.0, 1.0, 1.0], 5)
    assert w == 1  # the earliest of the two equal sums
    w, _ = ref.select([10, 10], [3.0, 3.0], 5)
    assert w == 0


def test_best_inlier_path_is_not_strict():
    w, _ = ref.select([3, 4, 4, 2], [1.0, 2.0, 3.0, 0.1], 5)
    assert w == 2  # the latest of the two highest counts
    w, _ = ref.select([0, 0, 0], [0.0, 0.0, 0.0], 5)
    assert w == 2


def test_best_inlier_path_is_frozen_once_a_licit_model_exists():
    w, _ = ref.select([3, 6, 4, 4], [1.0, 9.0, 1.0, 1.0], 5)
    assert w == 1  # the later, better-looking hypotheses with too few inliers change nothing
    w, _ = ref.select([4, 6, 7], [1.0, 9.0, 9.5], 5)
    assert w == 1


def test_given_model():
    w, _ = ref.select([10, 10], [2.0, 1.5], 5, given=(9, 1.5))
    assert w == -1  # licit and never beaten (a tie does not beat it)
    w, _ = ref.select([10, 10], [2.0, 1.4], 5, given=(9, 1.5))
    assert w == 1
    w, _ = ref.select([3, 4], [2.0, 1.0], 5, given=(4, 0.1))
    assert w == 1  # the given model is not licit: the best-inlier path, which it never enters
    w, _ = ref.select([], [], 5, given=(1, 0.1))
    assert w == -1  # no hypotheses: the given model, licit or not
    w, _ = ref.select([], [], 5)
    assert w is None


def test_abs_min_zero():
    assert ref.abs_min_of(0.0, 100) == 0 and ref.abs_min_of(0.004, 100) == 0 and ref.abs_min_of(0.006, 100) == 1
    assert ref.abs_min_of(-3.0, 100) == 0 and ref.abs_min_of(1.0, 65) == 65 and ref.abs_min_of(0.5, 5) == 3
    w, _ = ref.select([0, 0], [0.0, 0.0], 0)
    assert w == 0  # everything is licit; 0 < FLT_MAX, then 0 < 0 fails
    w, _ = ref.select([0, 2], [0.0, 0.5], 0, given=(0, 0.0))
    assert w == -1


# ---- conditions on the GPU tests' inputs -----------------------------------------------------------------------------------------

def _same_bits(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


def test_every_gpu_case_has_a_safe_decision_margin():
    """Two summation orders of n float64 terms differ by at most 2(n-1)*2^-53 relative (5e-12 at n = 33791): every `sum < best_sum`
    the restatement decides between models that are not bit-identical is decided by more than 1e-9 relative."""
    worst = 1.0
    for name, r, M_in in rc.all_margins():
        for h, s, best_sum, best in r["margins"]:
            if best is None:
                continue  # against the initial FLT_MAX
            holder = M_in if best == -1 else r["models"][best]
            if _same_bits(holder, r["models"][h]) and (best == -1 or r["singular"][best] == r["singular"][h]):
                continue
            top = max(abs(s), abs(best_sum))
            rel = abs(s - best_sum) / top if top > 0 else 0.0
            assert rel > 1e-9, (name, h, s, best_sum)
            worst = min(worst, rel)
    print("smallest decision margin: %.3g relative" % worst)


def test_cases_take_the_paths_they_are_meant_to():
    A, B, sets, r = rc.explicit_sets_case()
    assert r["singular"][1] and r["inliers"][2] == 0 and np.isnan(r["models"][3]).all() and r["inliers"][4] == 0 and r["winner"] in (0, 4)
    A, B, r = rc.best_inlier_tie_case()
    inl, w = r["inliers"][1:], r["winner"]
    assert (inl < ref.abs_min_of(1.0, len(B))).all() and inl[w] == inl.max()
    earlier = [h for h in range(w) if inl[h] == inl[w]]
    assert earlier and not any(_same_bits(r["models"][h], r["models"][w]) for h in earlier)
    A, B, M_in, r = rc.given_wins_case()
    assert r["winner"] == -1 and r["inliers"][0] == len(B) and (r["inliers"][1:] == len(B)).any() and _same_bits(r["M"], M_in)
    A, B, r = rc.iter2000_case()
    assert A.shape == (64 * 80, 3) and np.abs(r["M"] - np.array(rc.PLANE2000)).max() < 0.05
    wanted = {"all": 37 * 53, "none": 0, "column": 37}
    for name, c in rc.MASKED_CASES.items():
        want = rc.masked_case(name)[6]
        if c[2] in wanted and c[:2] == (37, 53):
            assert want[3] == wanted[c[2]], name
        assert want[2].shape == (c[0], c[1])
    assert rc.masked_case("checker_big_o1")[6][3] == 17000
    assert np.isnan(rc.masked_case("none_nogiven_o2")[6][1]).all()
    sizes = {c["ndata"] for c in rc.MATRIX_CASES.values()}
    assert {4, 7, 63, 64, 65, 255, 256, 257, 20011, rc.BIG_ROWS - 1, rc.BIG_ROWS, rc.BIG_ROWS + 1} <= sizes


def test_masked_data_is_column_major_with_one_based_coordinates():
    PHI = np.array([[1, -1, 0], [np.nan, 2, -0.0]], F32)
    D = np.arange(6, dtype=F32).reshape(2, 3)
    A, B = ref.masked_data(PHI, D, 1)
    assert A.tolist() == [[1, 1, 1], [2, 2, 1], [3, 1, 1], [3, 2, 1]] and B.tolist() == [0, 4, 2, 5]
    A2, _ = ref.masked_data(PHI, D, 2)
    assert A2[1].tolist() == [4, 4, 4, 2, 2, 1] and A2[2].tolist() == [9, 1, 3, 3, 1, 1]
    dist = ref.dist_plane(D, np.array([1, 10, 0], F32), 1)
    assert dist[1, 2] == (3 + 20 - 5) ** 2 and dist[0, 0] == 11 ** 2


# ---- the boundary ----------------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_entries(pdeip):
    syms = declared_symbols()
    lib = ctypes.CDLL(pdeip.capi.LIB_PATH)
    for name in ENTRIES:
        assert name in syms and hasattr(lib, name) and name in pdeip.capi.SIGNATURES, name


def _host_args(ndata=8, ncoef=3):
    A = np.ones((ndata, ncoef), F32, order="F")
    B = np.ones(ndata, F32)
    M = np.zeros(ncoef, F32)
    E = np.zeros(ndata, F32)
    return A, B, M, E


def test_c_abi_refuses_bad_arguments_without_a_gpu(pdeip):
    capi = pdeip.capi
    lib = capi.load()
    A, B, M, E = _host_args()
    a, b, m, e = (x.ctypes.data for x in (A, B, M, E))
    seed = ctypes.c_ulonglong(1)

    def host(A=a, B=b, ndata=8, ncoef=3, M_in=None, thr=0.5, mss=0.5, iter=3, sets=None, M_out=m, err=e):
        return lib.pdeip_surface_equation(A, B, ndata, ncoef, M_in, thr, mss, iter, sets, seed, M_out, err, None, None)

    def dev(A=a, B=b, ndata=8, ncoef=3, M_in=None, thr=0.5, mss=0.5, iter=3, sets=None, M_out=m, err=e):
        return lib.pdeip_surface_equation_dev(None, A, B, ndata, ncoef, M_in, thr, mss, iter, sets, seed, M_out, err, None, None)

    for fn in (host, dev):
        for kw, text in (({"A": None}, "'A' is NULL"), ({"B": None}, "'B' is NULL"), ({"M_out": None}, "'M_out' is NULL"),
                         ({"err": None}, "'err_out' is NULL"), ({"ncoef": 4}, "1st and 2nd order"), ({"ncoef": 0}, "1st and 2nd order"),
                         ({"ndata": 0}, "ndata must be >= 1"), ({"ndata": -5}, "ndata must be >= 1"),
                         ({"thr": float("inf")}, "err_thr must be finite"), ({"thr": float("nan")}, "err_thr must be finite"),
                         ({"mss": float("nan")}, "min_set_size must be finite"), ({"mss": float("-inf")}, "min_set_size must be finite"),
                         ({"iter": 0}, "nothing to return"), ({"iter": -2}, "nothing to return")):
            assert fn(**kw) == capi.PDEIP_ERR_ARG, (fn.__name__, kw)
            assert text in capi.last_error(), (fn.__name__, kw, capi.last_error())
    sets = np.array([[0, 1, 2, 3], [4, 5, 6, 8], [0, 0, 0, 0]], np.uint32)
    assert host(sets=sets.ctypes.data) == capi.PDEIP_ERR_ARG and "sets[7] = 8" in capi.last_error()

    P = np.ones((4, 5), F32, order="F")
    p = P.ctypes.data

    def masked(PHI=p, D=p, nrows=4, ncols=5, order=1, M_in=None, thr=0.5, mss=0.5, iter=3, M_out=m):
        return lib.pdeip_surface_fit_masked_dev(None, PHI, D, nrows, ncols, order, M_in, thr, mss, iter, None, seed, M_out, None, None)

    for kw, text in (({"PHI": None}, "'PHI' is NULL"), ({"D": None}, "'D' is NULL"), ({"M_out": None}, "'M_out' is NULL"),
                     ({"order": 0}, "order must be 1 or 2"), ({"order": 3}, "order must be 1 or 2"), ({"nrows": 0}, "must not be empty"),
                     ({"thr": float("nan")}, "err_thr must be finite"), ({"mss": float("inf")}, "min_set_size must be finite"),
                     ({"iter": 0}, "nothing to return")):
        assert masked(**kw) == capi.PDEIP_ERR_ARG, kw
        assert text in capi.last_error(), (kw, capi.last_error())


def test_stub_refuses_what_the_reference_gateway_refuses(pdeip):
    lib = rc.build_seg_stub("SurfaceEquation", pdeip)
    A = np.ones((8, 3), F32)
    B = np.ones((8, 1), F32)
    M = np.zeros((3, 1), F32)
    good = [A, B, M, F32(0.5), F32(0.5), F32(3)]
    for args in (good[:5], good + [np.float64(1), np.float64(2)]):
        err, _ = call(lib, 2, args)
        assert err == "SurfaceEquation error: wrong number of input parameters!"
    for k, name in enumerate(("A_in", "B_in", "M_in")):
        bad = list(good)
        bad[k] = bad[k].astype(np.float64)
        err, _ = call(lib, 2, bad)
        assert err == "SurfaceEquation error: '%s' must be a noncomplex single-valued matrix." % name
    for k, name in ((3, "err_thr"), (4, "min_set_size"), (5, "iter")):
        bad = list(good)
        bad[k] = np.float64(1)
        err, _ = call(lib, 2, bad)
        assert err == "SurfaceEquation error: '%s' must be a noncomplex, single-type scalar" % name
    err, _ = call(lib, 2, [A, B, np.zeros((6, 1), F32)] + good[3:])
    assert err == "SurfaceEquation error: M_in is a column vector with as many row elements as A_in has columns!"
    err, _ = call(lib, 2, [A, np.ones((7, 1), F32)] + good[2:])
    assert err == "SurfaceEquation error: A_in and B_in have to have same amount of rows!"
    err, _ = call(lib, 2, [np.ones((8, 4), F32), B, np.zeros((4, 1), F32)] + good[3:])
    assert err == "SurfaceEquation error: only 1st and 2nd order polynomials are implemented!"
    err, _ = call(lib, 1, good)
    assert err == "SurfaceEquation error: insufficient number of outputs. Outputs from this function is 'M_out' and 'error_out'"
    err, _ = call(lib, 2, good + [np.float64(-1)])
    assert err == "SurfaceEquation error: 'seed' must be in 0 .. 2^64 - 1"
    err, _ = call(lib, 2, good + [np.zeros((2, 1))])
    assert err == "SurfaceEquation error: 'seed' must be a real scalar"
    # refused by the library before any HIP call: a non-finite threshold; no hypotheses and an empty M_in
    err, _ = call(lib, 2, [A, B, M, F32(np.inf), F32(0.5), F32(3), np.float64(1)])
    assert "err_thr must be finite" in err
    err, _ = call(lib, 2, [A, B, np.zeros((0, 0), F32), F32(0.5), F32(0.5), F32(0), np.float64(1)])
    assert "nothing to return" in err


def test_mex_api_checks(pdeip):
    api = pdeip.mex_api
    A = np.ones((8, 3), F32)
    B = np.ones((8, 1), F32)
    M = np.zeros((3, 1), F32)
    with pytest.raises(api.MexError, match="'B_in' must be a noncomplex single-valued matrix"):
        api.SurfaceEquation(A, B.astype(np.float64), M, F32(0.5), F32(0.5), F32(3), seed=1)
    with pytest.raises(api.MexError, match="'iter' must be a noncomplex, single-type scalar"):
        api.SurfaceEquation(A, B, M, F32(0.5), F32(0.5), 3, seed=1)
    with pytest.raises(api.MexError, match="same amount of rows"):
        api.SurfaceEquation(A, B[:7], M, F32(0.5), F32(0.5), F32(3), seed=1)
    with pytest.raises(api.MexError, match="only 1st and 2nd order"):
        api.SurfaceEquation(np.ones((8, 5), F32), B, np.zeros((5, 1), F32), F32(0.5), F32(0.5), F32(3), seed=1)
    with pytest.raises(api.MexError, match="insufficient number of outputs"):
        api.SurfaceEquation(A, B, M, F32(0.5), F32(0.5), F32(3), seed=1, nargout=1)
    with pytest.raises(api.MexError, match="sets\\[4\\] = 9"):
        api.SurfaceEquation(A, B, M, F32(0.5), F32(0.5), F32(2), sets=np.array([[0, 1, 2, 3], [9, 1, 2, 3]], np.uint32))
