"""CPU: every case of tests/levelset_cases.py is what its name says.

The GPU tests (test_gpu_gac_stages.py, test_gpu_line_edges.py) only consume the cases; what a case contains -- the rank at which
MATLAB's round() and integer arithmetic part, the neighbours of a selected value, the zero count of Igrad around the rank, the share
of a reference output that is finite -- is proved here, against numpy alone."""
import math

import numpy as np
import pytest

import diffusion_ref
import levelset_cases as lc
import levelset_ref as ref

F32 = np.float32


# ---- the rank --------------------------------------------------------------------------------------------------------------------

def test_the_drivers_rank_is_the_rounded_double_product():
    """round(0.7*N) on the double product: 31, 59 and 115 at N = 45, 85 and 165, where (7N+5)/10 gives one more."""
    assert [lc.driver_rank(n) for n in lc.ROUND_N] == [31, 59, 115]
    assert [lc.exact_rank(n) for n in lc.ROUND_N] == [32, 60, 116]
    assert 0.7 * 45 == 31.499999999999996
    part = [n for n in range(1, 400000) if lc.driver_rank(n) != lc.exact_rank(n)]
    assert len(part) == 9362 and part[:5] == [45, 85, 165, 175, 325]
    # floor(x + 0.5) is how the restatement writes MATLAB's round; C's round() on the same double (the host code) agrees everywhere
    assert all(lc.driver_rank(n) == max(int(round_half_away(0.7 * n)), 1) for n in range(1, 400000))
    assert all(lc.driver_rank(n) == int(math.floor(0.7 * n + 0.5)) for n in lc.SEL_SIZES if n > 1)


def round_half_away(x):
    """C's round() for x >= 0 without an addition that could round: the integer part, plus one when the fraction reaches a half."""
    f = math.floor(x)
    return f + 1 if x - f >= 0.5 else f  # x - f is exact for doubles below 2^52


@pytest.mark.parametrize("n", lc.ROUND_N)
def test_an_off_by_one_rank_changes_the_answer_where_the_roundings_part(n):
    x, k, _ = lc.selection_cases()["round_n%d_sensitive" % n]
    Y = np.sort(x)
    assert k == lc.driver_rank(n) and lc.exact_rank(n) == k + 1
    assert Y[k - 1] != Y[k] and Y[k - 2] != Y[k - 1]
    assert ref.gac_lambda(x) == Y[k - 1]  # the restatement takes the same rank


# ---- the selection cases ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", lc.SELECTION_NAMES)
def test_selection_case_is_rank_sensitive_or_named_as_tied(name):
    x, k, zero = lc.selection_cases()[name]
    assert x.ndim == 1 and x.dtype == F32 and not x.flags.writeable and 1 <= k <= x.size
    Y = np.sort(x)
    me = Y[k - 1]
    nb = [Y[j] for j in (k - 2, k) if 0 <= j < Y.size]
    differ = [not (lc.same(v, me) or (v == 0 and me == 0)) for v in nb]
    kind = name.rsplit("_", 1)[1]
    assert kind in ("sensitive", "edge", "tied")
    if kind == "sensitive":
        assert all(differ)
    elif kind == "edge":
        assert any(differ) and not all(differ)
    else:
        assert not any(differ) and nb
    # compared by value exactly where the selected element is a zero of a plateau that holds both signs
    zeros = x[x == 0]
    mixed = me == 0 and np.signbit(zeros).any() and not np.signbit(zeros).all()
    assert zero == bool(mixed)


def test_selection_cases_cover_the_sizes_the_ranks_and_the_contents():
    T = lc.selection_cases()
    sizes = {x.size for x, _, _ in T.values()}
    assert set(lc.SEL_SIZES) <= sizes and lc.SEL_SIZES[-4:] == (262143, 262144, 262145, 262144 + 257)
    for n in lc.SEL_SIZES:
        ranks = {k for x, k, _ in T.values() if x.size == n}
        assert {1, n, lc.driver_rank(n)} <= ranks, n

    def picked(name):
        x, k, _ = T[name]
        return np.sort(x)[k - 1]

    tiny = F32(2.0 ** -126)
    assert picked("mixed_neg_normal_sensitive") <= -1 and picked("mixed_pos_normal_sensitive") >= 1
    assert -tiny < picked("mixed_neg_subnormal_sensitive") < 0 < picked("mixed_pos_subnormal_sensitive") < tiny
    assert picked("mixed_last_negative_sensitive") == -F32(1.4e-45) and picked("mixed_first_positive_sensitive") == F32(1.4e-45)
    assert picked("inf_first_sensitive") == -np.inf and picked("inf_last_tied") == np.inf and picked("inf_first_posinf_edge") == np.inf
    assert np.isfinite(picked("inf_after_neginf_sensitive")) and np.isfinite(picked("inf_before_posinf_sensitive"))
    assert np.isfinite(picked("nan_below_sensitive")) and np.isfinite(picked("nan_last_number_sensitive"))
    for name in ("nan_first_nan_edge", "nan_inside_tied", "nan_last_tied", "nan_and_inf_edge", "all_nan_tied", "one_nan_sensitive"):
        assert np.isnan(picked(name)), name
    x, k, _ = T["nan_and_inf_edge"]
    assert np.sort(x)[k - 2] == np.inf
    x, _, _ = T["all_equal_tied"]
    assert (x == x[0]).all()
    x, k, _ = T["two_values_last_of_lower_edge"]
    assert set(x.tolist()) == {0.25, 0.5} and np.sort(x)[k - 1] == 0.25 and np.sort(x)[k] == 0.5
    x, k, _ = T["two_values_first_of_upper_edge"]
    assert np.sort(x)[k - 1] == 0.5 and np.sort(x)[k - 2] == 0.25
    for name in ("zeros_first_edge", "zeros_lower_half_tied", "zeros_upper_half_tied", "zeros_last_edge"):
        assert picked(name) == 0 and T[name][2], name
    x, _, _ = T["zeros_first_edge"]
    assert (np.signbit(x) & (x == 0)).sum() == 150 and (~np.signbit(x) & (x == 0)).sum() == 150
    # the second trip of the histogram's grid-stride loop decides alone: every element of the first trip is above the answer
    x, k, _ = T["second_trip_only_sensitive"]
    assert x.size == lc.HIST_SPAN + 257 and (x[:lc.HIST_SPAN] == 2).all() and (x[lc.HIST_SPAN:] < 0).all()
    assert np.sort(x)[k - 1] == x[lc.HIST_SPAN:].max() and k == 257
    assert picked("second_trip_count_edge") == 2  # a histogram that loses the second trip finds 2.0 at rank 257 already
    assert np.sort(x[:lc.HIST_SPAN])[k - 1] == 2


# ---- the stopping function and the drivers ---------------------------------------------------------------------------------------

def test_patch_sizes_straddle_the_rank():
    """The flat 40x50 image with a noise patch in its corner: the zero count of Igrad is just below, equal to and just above the rank
    1400 at the patch sizes the case names record, and lambda is the first non-zero value, zero and zero."""
    k = lc.driver_rank(2000)
    assert k == 1400
    assert lc.patch_search() == (lc.PATCH_BELOW, lc.PATCH_EQUAL, lc.PATCH_ABOVE)
    counts = [lc.patch_zero_count(*p) for p in (lc.PATCH_BELOW, lc.PATCH_EQUAL, lc.PATCH_ABOVE)]
    assert counts == [1399, 1400, 1401]
    assert lc.patch_zero_count(8, 8) == 1857 and lc.patch_zero_count(21, 21) == 1376
    for tag, p, zero_lambda in (("below", lc.PATCH_BELOW, False), ("equal", lc.PATCH_EQUAL, True), ("above", lc.PATCH_ABOVE, True)):
        name = "patch%dx%d_zeros_%s_rank_40x50x1" % (p + (tag,))
        _, Igrad, lam = lc.want_stopping(name, -1.0)
        assert (lam == 0) == zero_lambda, name
        if not zero_lambda:
            assert lam == np.sort(Igrad.ravel())[1399] and lam == Igrad[Igrad > 0].min()
    assert float(lc.want_stopping("patch21x21_40x50x1", -1.0)[2]) == pytest.approx(3.87e-05, rel=0.01)
    assert lc.want_stopping("patch8x8_40x50x1", -1.0)[2] == 0


def test_images_hold_what_their_names_say():
    T = lc.images()
    for name, I in T.items():
        shape = tuple(int(v) for v in name.rsplit("_", 1)[1].split("x"))
        assert I.shape == (shape if shape[2] > 1 else shape[:2]) and I.dtype == F32 and not I.flags.writeable, name
    shapes = {I.shape[:2] for I in T.values()}
    assert {(3, 3), (3, 7), (7, 3), (5, 9), (65, 7), (7, 257), (255, 4), (257, 4), (513, 512)} <= shapes
    assert {1, 2, 3} <= {(I.shape[2] if I.ndim == 3 else 1) for I in T.values()}
    assert 513 * 512 > lc.HIST_SPAN and 5 * 9 == 45
    for name in ("binary_65x7x1", "binary_33x31x3"):
        assert set(np.unique(T[name]).tolist()) == {0.0, 1.0}
        Igrad = lc.want_stopping(name, -1.0)[1]
        assert np.unique(Igrad).size < Igrad.size // 2  # ties
    assert set(np.unique(T["step_33x31x1"]).tolist()) == {0.0, 1.0} and lc.want_stopping("step_33x31x1", -1.0)[2] == 0
    assert (T["flat_40x50x1"] == 0.25).all() and (lc.want_stopping("flat_40x50x1", -1.0)[1] == 0).all()
    assert np.isnan(T["one_nan_65x31x1"]).sum() == 1 and np.isnan(T["one_nan_33x31x3"]).sum() == 1
    g, Igrad, lam = lc.want_stopping("one_nan_65x31x1", -1.0)
    assert 0 < np.isnan(Igrad).sum() < Igrad.size and np.isfinite(lam) and np.array_equal(np.isnan(g), np.isnan(Igrad))
    for c in (0, 1, 2):  # one channel all NaN: max(., [], 3) drops it, so nothing of it reaches Igrad
        I = T["nan_channel%d_33x31x3" % c]
        assert np.isnan(I[:, :, c]).all() and np.isfinite(np.delete(I, c, axis=2)).all()
        assert np.isfinite(lc.want_stopping("nan_channel%d_33x31x3" % c, -1.0)[1]).all()
    g, Igrad, lam = lc.want_stopping("all_nan_9x11x2", -1.0)
    assert np.isnan(Igrad).all() and np.isnan(lam) and np.isnan(g).all()


def test_stopping_cases_cover_the_given_lambdas():
    given = {lam for _, lam in lc.STOPPING if lam >= 0 or (lam == 0 and np.signbit(lam))}
    assert {0.002, 0.0, 1e-40} <= given
    assert 0 < F32(1e-40) < F32(2.0 ** -126)  # a subnormal single
    assert lc.want_stopping("noise_65x7x3", 1e-40)[2] == F32(1e-40)
    g = lc.want_stopping("noise_65x7x3", 0.0)[0]
    assert (g == 0).all()  # 1/(1 + x/0) = 1/Inf
    # model a's flooding inputs are pinned here: lambda = 0 next to zeros of Igrad gives 0/0
    for name in ("flat_40x50x1", "step_33x31x1", "patch8x8_40x50x1", "one_nan_65x31x1"):
        assert (name, -1.0) in lc.STOPPING and np.isnan(lc.want_stopping(name, -1.0)[0]).any()


def test_driver_cases_cover_the_parameters():
    prm = [dict(p) for _, _, p in lc.DRIVER_RUNS]
    assert all(p["ITER"] <= 3 for p in prm)
    assert {p.get("c", -0.1) for p in prm} >= {-0.1, 0.0, 0.1}
    assert {p.get("tau", 0.25) for p in prm} >= {0.25, 0.1}
    assert {p.get("SMOOTH", 100) for p in prm} >= {100, 1}
    assert {p["ITER"] for p in prm} >= {0, 0.5, 2.5}
    assert {p.get("lam", -1.0) for p in prm} >= {-1.0, 0.002, 0.0, 1e-40}
    assert [dict(p)["ITER"] for img, _, p in lc.DRIVER_RUNS if img == "noise_513x512x1"] == [1, 1]
    assert {img for img, _, _ in lc.DRIVER_RUNS} >= {n for n in lc.IMAGE_NAMES if n.startswith("noise_")}


@pytest.mark.parametrize("run", lc.DRIVER_RUNS, ids=lc.driver_id)
def test_driver_reference_is_informative(run):
    """At least 75 % of the reference output is finite, so that a comparison in which any NaN equals any NaN still proves something."""
    want = lc.want_gac(*run)
    assert want.shape == lc.images()[run[0]].shape[:2]
    assert lc.finite_share(want) >= 0.75, lc.finite_share(want)
    if dict(run[2])["ITER"] > 0:
        assert not np.array_equal(want, ref.Reinit(lc.phi_for(run[0]), F32(10)))  # the iterations did something


def test_model_a_floods_where_model_b_does_not():
    """lambda = 0 beside zeros of Igrad, or a NaN in g: model a's output is NaN everywhere (the cases run model b only; model a's
    inputs are pinned through the stopping function), and one driver case pins the flood itself."""
    for img, models, prm in lc.DRIVER:
        if models == "b":
            a = ref.GAC(lc.images()[img], lc.phi_for(img), "a", **prm)
            assert lc.finite_share(a) < 0.75, img
    img, model, prm = lc.FLOOD
    assert np.isnan(lc.want_gac(img, model, tuple(sorted(prm.items())))).all()


# ---- the line solves -------------------------------------------------------------------------------------------------------------

def test_chunk_shapes_put_the_line_ends_on_the_chunk_edges():
    lengths = {n for s in lc.CHUNK_SHAPES for n in s}
    assert {9, 10, 11, 18, 2, 66} == lengths
    assert {(n - 2) % lc.CHUNK for n in lengths if n > 2} >= {0, 1, 7}   # the forward chunk ends on, one past and one short of n-2
    assert {(n - 1) % lc.CHUNK for n in lengths} >= {0, 1, 2}             # the backward chunk exactly full, one and two over
    assert (10 - 2) % 8 == 0 and (18 - 2) % 8 == 0 and (66 - 2) % 8 == 0 and (9 - 1) % 8 == 0
    assert len(lc.CHUNK_SHAPES) == 20 and len(set(lc.CHUNK_SHAPES)) == 20


@pytest.mark.parametrize("family", ["ac", "cv", "d4"])
def test_chunk_references_are_finite(family):
    for shape in lc.CHUNK_SHAPES:
        prob = lc.chunk_problem(family, shape)
        assert all(x.shape == shape + (3,) and np.isfinite(x).all() for x in prob)
        if family == "d4":
            want = diffusion_ref.Diffusion4_v10(prob[0])
        else:
            want = lc.solve_ref(family, prob, *(lc.AC_TAU_NU if family == "ac" else lc.CV_TAU_NU))
        assert np.isfinite(want).all(), shape


@pytest.mark.parametrize("family", ["ac", "cv"])
@pytest.mark.parametrize("case", lc.RANGE_CASES, ids=lc.range_id)
def test_range_case_holds_its_value_and_stays_informative(family, case):
    plane, value, how = case
    prob, base = lc.range_problem(family, *case), lc.range_base(family)
    hit = prob[plane].view(np.uint32) == np.asarray(value, F32).view(np.uint32)
    changed = prob[plane].view(np.uint32) != base[plane].view(np.uint32)
    assert (changed <= hit).all() and changed.any()
    if how == "laced":
        per_frame = hit.reshape(-1, 3).sum(axis=0)
        assert (per_frame >= 6).all() and 0.015 <= changed.mean() <= 0.06
    else:
        assert changed.sum() == 1 and changed[lc.RANGE_PIXEL]
    for k in range(4):
        if k != plane:
            assert np.array_equal(prob[k].view(np.uint32), base[k].view(np.uint32))
    tn = lc.AC_TAU_NU if family == "ac" else lc.CV_TAU_NU
    want = lc.solve_ref(family, prob, *tn)
    assert lc.finite_share(want) >= 0.75, lc.finite_share(want)
    assert not np.array_equal(want.view(np.uint32), lc.solve_ref(family, base, *tn).view(np.uint32))  # the value reaches the output


@pytest.mark.parametrize("family", ["ac", "cv"])
def test_tau_nu_cases_stay_finite(family):
    for tau, nu in lc.TAU_NU_CASES:
        assert np.isfinite(lc.solve_ref(family, lc.range_base(family), tau, nu)).all(), (tau, nu)
    assert 0 < F32(1e-40) < F32(2.0 ** -126)


def test_diffusion_range_cases_stay_finite():
    for v in lc.DIFF_VALUES:
        I = lc.diff_laced(v)
        hit = (I.view(np.uint32) == np.asarray(v, F32).view(np.uint32)).all(axis=2)
        assert 3 <= hit.sum() <= 12, (v, int(hit.sum()))
        assert np.isfinite(diffusion_ref.Diffusion4_v10(I)).all(), v
    I = lc.diff_image(301, lc.DIFF_SHAPE)
    for alpha in lc.DIFF_ALPHAS:
        assert np.isfinite(diffusion_ref.Diffusion4_v10(I, alpha=alpha)).all(), alpha
    assert not np.isfinite(diffusion_ref.Diffusion4_v10(I, alpha=1e10)).any()  # why alpha >= 1e10 is left out


@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
def test_one_bad_pixel_stays_in_its_row_and_column_for_one_diffusion_iteration(value):
    I = lc.diff_one_pixel(value)
    bad_in = ~np.isfinite(I)
    assert bad_in.sum() == 1 and bad_in[lc.DIFF_PIXEL]
    out = diffusion_ref.Diffusion4_v10(I, outer_iter=0)
    assert diffusion_ref.iterations(0) == 1
    i, j, c = lc.DIFF_PIXEL
    bad = np.argwhere(~np.isfinite(out))
    assert len(bad) > 0 and all((b[0] == i or b[1] == j) and b[2] == c for b in bad)
    assert lc.finite_share(out) >= 0.75


def test_a_flat_image_does_not_come_back_flat():
    out = diffusion_ref.Diffusion4_v10(lc.diff_flat())
    dev = float(np.abs(out - F32(77.25)).max())
    assert np.isfinite(out).all() and 0 < dev <= 0.0125, dev


def test_reinit_cases():
    P = lc.reinit_step_case()
    for v in lc.REINIT_STEP_VALUES:
        assert (P.view(np.uint32) == np.asarray(v, F32).view(np.uint32)).sum() >= 3, v
    one = ref.Reinit(P, F32(0.25))
    assert ref.reinit_steps(0.25) == 1 and 0.75 <= lc.finite_share(one) < 1
    # a single step does not carry a non-finite value beyond radius 1 of a laced pixel
    src = ~np.isfinite(P) | (np.abs(P) >= F32(1e18))
    near = src.copy()
    near[1:] |= src[:-1]
    near[:-1] |= src[1:]
    near[:, 1:] |= src[:, :-1]
    near[:, :-1] |= src[:, 1:]
    assert (~np.isfinite(one) <= near).all()
    Q = lc.reinit_long_case()
    for v in lc.REINIT_LONG_VALUES:
        assert (Q.view(np.uint32) == np.asarray(v, F32).view(np.uint32)).sum() >= 3, v
    assert np.isfinite(ref.Reinit(Q, F32(10))).all() and ref.reinit_steps(10) == 40
