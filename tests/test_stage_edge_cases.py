"""CPU: every case of tests/stage_edge_cases.py is what its name says (a case that is not would pass while testing nothing), the
numpy statement of the lambda selection agrees with an independent second statement, and the three places where the statement of
oracle/matlab_side.py and MATLAB's documented semantics are settled: NaN orders above +Inf in the median, max over the frames
skips NaN, and an all-NaN pixel carries NaN into the selection."""
import numpy as np
import pytest

import stage_edge_cases as sc

pytestmark = pytest.mark.filterwarnings("ignore:invalid value encountered:RuntimeWarning")  # Inf - Inf, NaN on purpose
ms = sc.matlab_side()
F32 = np.float32


def nan_equal_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(na, nb) and np.array_equal(a[~na].view(u), b[~nb].view(u))


# ---- median cases ----------------------------------------------------------------------------------------------------------------

def test_median_case_names_are_unique_and_cases_are_read_only():
    names = sc.median_names()
    assert len(set(names)) == len(names)
    for _, S, A, B, _ in sc.median_cases():
        for a in (S, A, B):
            assert not a.flags.writeable and a.dtype == np.float32


@pytest.mark.parametrize("name", sc.median_names())
def test_median_case_contains_the_windows_it_claims(name):
    _, S, _, _, kinds = sc.median_case(name)
    have = sc.median_kinds(S)
    assert kinds <= have, "%s lacks %s" % (name, sorted(kinds - have))
    if name.startswith("nan_"):
        assert {"nan%d" % k for k in sc.NAN_COUNTS} <= kinds  # windows with exactly 0, 1, 4, 5 and 9 NaN


def test_median_cases_cover_every_kind_of_window():
    claimed = set().union(*[c[4] for c in sc.median_cases()])
    assert set(sc.MEDIAN_KINDS) <= claimed
    shapes = {c[1].shape for c in sc.median_cases()}
    assert (300, 3) in shapes and (3, 3) in shapes and any(r == 3 and c > 3 for r, c in shapes)  # the 256-row block; the smallest frames


@pytest.mark.parametrize("name", sc.median_names())
def test_median_case_two_term_form_sums_to_the_frame(name):
    _, S, A, B, _ = sc.median_case(name)
    with np.errstate(invalid="ignore"):
        assert nan_equal_bits((A + B).astype(F32), S)
    assert not np.array_equal(A.view(np.uint32), S.view(np.uint32)) or S.size <= 9  # B really contributes
    assert nan_equal_bits(ms.median3_sum(A, B), ms.median3_sum(S))


@pytest.mark.parametrize("name", sc.median_names())
def test_median_statement_is_the_fifth_of_the_nan_last_order(name):
    """np.sort's order spelled out: numbers ascending (-Inf first, +Inf last), then NaN; k NaN in the window leave the 5th smallest
    number for k <= 4 and NaN for k >= 5."""
    _, S, _, _, _ = sc.median_case(name)
    W = sc.windows(S)
    want = np.empty(S.shape, F32)
    for i in range(S.shape[0]):
        for j in range(S.shape[1]):
            w = W[:, i, j]
            nums = sorted(float(x) for x in w[~np.isnan(w)])
            want[i, j] = nums[4] if len(nums) >= 5 else np.nan
    got = ms.median3_sum(S)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])  # by value: -0 == +0


@pytest.mark.parametrize("name", sc.median_names())
def test_exchange_network_with_the_nan_aware_rule_selects_the_median(name):
    """The kernel's 19 exchanges with 'exchange if a > b or a is NaN' give the statement's bits, except for the sign of a zero median
    of a window that holds both zeros (compared by value there: the contract leaves that sign open)."""
    _, S, _, _, _ = sc.median_case(name)
    got, want = sc.median_model(S), ms.median3_sum(S)
    loose = sc.mixed_zero_median(S)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got[loose], want[loose])
    assert nan_equal_bits(got[~loose], want[~loose])


def test_min_max_exchange_would_lose_nan():
    """What the case list is for: an exchange by fmin / fmax (which return the number of a number-NaN pair) differs from the statement
    on windows with NaN, in finite values (1..4 NaN) and in NaN positions (5 or more)."""
    _, S, _, _, _ = sc.median_case("nan_counts_23x21")
    v = list(sc.windows(S))
    for a, b in ((1, 2), (4, 5), (7, 8), (0, 1), (3, 4), (6, 7), (1, 2), (4, 5), (7, 8), (0, 3), (5, 8), (4, 7), (3, 6), (1, 4), (2, 5), (4, 7),
                 (4, 2), (6, 4), (4, 2)):
        v[a], v[b] = np.fmin(v[a], v[b]), np.fmax(v[a], v[b])
    want = ms.median3_sum(S)
    assert not np.array_equal(np.isnan(v[4]), np.isnan(want))
    both = ~np.isnan(v[4]) & ~np.isnan(want)
    assert (v[4][both] != want[both]).any()


# ---- selection cases -------------------------------------------------------------------------------------------------------------

def test_selection_case_names_are_unique_and_every_seam_has_both_classes_in_both_forms():
    names = sc.selection_names()
    assert len(set(names)) == len(names)
    for shape in sc.SEAM_SHAPES:
        for form in (None, "q"):
            classes = {cls for _, D, q, cls in sc.selection_cases() if D.shape[:2] == shape and (q is None) == (form is None)}
            assert {"rank", "tie"} <= classes, (shape, form)
    sizes = [r * c for r, c in sc.SEAM_SHAPES]
    assert sizes == [4096, 4097, 16384, 16385, 40000]
    assert all(r <= 200 and c <= 200 or r * c <= 40000 for r, c in sc.SEAM_SHAPES)


@pytest.mark.parametrize("name", sc.selection_names())
def test_selection_case_is_of_its_class(name):
    _, D, q, cls = sc.selection_case(name)
    assert not D.flags.writeable
    assert cls in ("rank", "tie")
    assert sc.classify(D, q) == cls


@pytest.mark.parametrize("name", sc.selection_names())
def test_sort_and_index_equals_partition(name):
    """An independent second statement of the selection: np.partition at the same rank (an introselect, no full sort)."""
    _, D, q, _ = sc.selection_case(name)
    info = sc.selection_info(D, q)
    norm = info["norm"].ravel()
    nz = norm[norm != 0]
    assert nz.size == info["sorted"].size and info["rank"] == ms.ad_rank(nz.size, q)
    second = np.partition(nz, info["rank"] - 1)[info["rank"] - 1]
    assert nan_equal_bits(np.float64(second), np.float64(info["lam"]))
    assert nan_equal_bits(np.float64(ms.ad_diff_weights(D, q)[1]), np.float64(info["lam"]))


def test_rank_ends_and_crossing():
    D = sc.selection_case("random_113x145_q_one")[1]
    srt = sc.selection_info(D, 1.0)["sorted"]
    assert sc.selection_info(D, 1.0)["rank"] == srt.size and sc.selection_info(D, 1.0)["lam"] == srt[-1]   # the largest norm
    q = sc.selection_case("random_113x145_q_clamped")[2]
    assert np.floor(srt.size * q + 0.5) == 0 and sc.selection_info(D, q)["rank"] == 1                     # the rank clamps to 1
    below, above = sc.selection_case("random_113x145_q_below_crossing")[2], sc.selection_case("random_113x145_q_above_crossing")[2]
    assert np.nextafter(below, 1.0) == above                                                               # adjacent doubles
    assert (sc.selection_info(D, below)["rank"], sc.selection_info(D, above)["rank"]) == (7000, 7001)
    assert srt[6999] != srt[7000]


def test_three_frame_case_has_changing_strongest_frames_and_exact_ties_that_show():
    D = sc.selection_case("frames3_113x145_q90")[1]
    gx, gy = ms.ad_frame_gradients(D)
    nn = gx * gx + gy * gy
    first = ms.matlab_max_index(nn)
    assert all((first == f).mean() > 0.2 for f in range(3))                   # every frame is the strongest on a good part of the frame
    assert (first[:, 1:] != first[:, :-1]).mean() > 0.3                       # and that changes from pixel to pixel
    top = nn.max(axis=2)
    tied = (nn == top[:, :, None]) & (top[:, :, None] > 0)
    assert int((tied.sum(axis=2) == 3).sum()) >= 9                            # the impulses: all three frames tie exactly
    last = 2 - np.argmax(nn[:, :, ::-1], axis=2)                              # the LAST maximal frame instead of the first
    assert ((last != first) & (top > 0)).sum() >= 9
    for q in (0.9, None):
        info = sc.selection_info(D, q)
        mx, my, norm = ms.ad_strongest(gx, gy, last)
        assert np.array_equal(norm, info["norm"])                             # the same norms, hence the same lambda ...
        other = dict(info, mx=mx, my=my)
        a, b = sc.weights_with(info, info["lam"], q, 500.0), sc.weights_with(other, info["lam"], q, 500.0)
        assert any(not np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))   # ... but other weights


def test_a_flat_image_that_is_not_zero_leaves_a_rounding_residue():
    info = sc.selection_info(sc.selection_case("flat_residue_128x128_q90")[1], 0.9)
    assert info["sorted"].size == 128 * 128 and 0 < info["lam"] < 1e-30 and (info["sorted"] == info["lam"]).all()
    assert (info["mx"] == 0).all() and (info["my"] != 0).all()


def test_degenerate_cases_have_the_norms_they_claim():
    for name, D, nonzero in sc.degenerate_cases():
        info = sc.selection_info(D, 0.9)
        assert info["sorted"].size == nonzero, name
        if nonzero == 0:
            assert info["lam"] == 1.0 and ms.ad_diff_weights(D, None)[1] == 1.0
        else:
            ii, jj = np.nonzero(info["norm"])
            assert ii.max() - ii.min() == 2 and jj.max() - jj.min() == 2      # one pixel's neighbourhood


# ---- NaN and Inf: the frame maximum ---------------------------------------------------------------------------------------------

def test_nonfinite_cases_are_what_they_claim():
    for name, D, what in sc.nonfinite_cases():
        D3 = D if D.ndim == 3 else D[:, :, None]
        gx, gy = ms.ad_frame_gradients(D)
        nan = np.isnan(gx * gx + gy * gy)
        if what == "all":
            assert nan.all(axis=2).any(), name
        if what == "some":
            assert (nan.any(axis=2) & ~nan.all(axis=2)).any() and not nan.all(axis=2).any(), name
            assert (nan.sum(axis=2) == 2).any() and nan[:, :, 0].any()        # two of three; and a NaN in the first frame
        if what == "inf":
            assert np.isinf(D3).any() and not np.isnan(D3).any() and nan.any() and np.isinf(gx * gx + gy * gy).any(), name


def test_frame_maximum_follows_matlab_max():
    """max(A, [], 3) ignores NaN; the index is that of the first maximal number, or the first frame where every frame is NaN."""
    nan = np.nan
    A = np.array([[[1.0, 3.0, 3.0], [nan, 2.0, 5.0], [nan, nan, nan], [4.0, nan, 4.0], [nan, 0.0, nan], [np.inf, nan, np.inf]]])
    assert ms.matlab_max_index(A).tolist() == [[1, 2, 0, 0, 1, 0]]
    assert nan_equal_bits(ms.matlab_max(A), np.array([[3.0, 5.0, nan, 4.0, 0.0, np.inf]]))


def test_ad_statement_skips_nan_frames_and_carries_all_nan_pixels():
    _, D, _ = [c for c in sc.nonfinite_cases() if c[0] == "nan_some_frames_64x67x3"][0]
    mx, my, norm = ms.ad_strongest(*ms.ad_frame_gradients(D))
    assert not np.isnan(norm).any()                                            # a NaN in some frames is skipped
    gx, gy = ms.ad_frame_gradients(D)
    assert np.isnan(ms.ad_strongest(gx, gy, np.argmax(gx * gx + gy * gy, axis=2))[2]).any()   # np.argmax would have taken it
    for name in ("nan_single_frame_64x64", "nan_every_frame_64x67x3"):
        D = [c for c in sc.nonfinite_cases() if c[0] == name][0][1]
        info = sc.selection_info(D, 1.0)
        assert np.isnan(info["norm"]).any() and np.isnan(info["sorted"][-1]) and np.isnan(info["lam"])   # non-zero and the largest
        assert np.isfinite(sc.selection_info(D, 0.9)["lam"])
        assert info["sorted"].size == D.shape[0] * D.shape[1]                  # counted among the non-zero norms


def test_tv4_statement_skips_nan_frames():
    D = [c for c in sc.nonfinite_cases() if c[0] == "nan_some_frames_64x67x3"][0][1]
    w = ms.tv4_diff_weights(D)
    one_of_three = np.isnan(D).sum(axis=2) == 1
    assert one_of_three.any()
    # the NaN reaches the weights of the pixel and its neighbours in that frame only: the other frames decide, no weight is NaN
    assert not any(np.isnan(a).any() for a in w)
    every = [c for c in sc.nonfinite_cases() if c[0] == "nan_every_frame_64x67x3"][0][1]
    assert any(np.isnan(a).any() for a in ms.tv4_diff_weights(every))          # NaN in every frame does come through


# ---- warps -------------------------------------------------------------------------------------------------------------------------

def test_sym_warp_cases_hit_the_ends_exactly_and_by_one_ulp():
    for name, U, Uq in sc.sym_warp_cases():
        rows, cols = U.shape
        xq = np.arange(1, cols + 1, dtype=np.float64)[None, :] + Uq.astype(np.float64)
        want = ms.sym_warp_flow(U, Uq)
        for x in (1.0, float(cols), float(sc.ulp_down(1.0))):
            assert (xq == x).any(), (name, x)
        assert np.isnan(xq).any() and (xq == np.inf).any() and (xq == -np.inf).any()
        assert np.isnan(want[xq == float(sc.ulp_down(1.0))]).all() and not np.isnan(want[xq == 1.0]).any()
        assert not np.isnan(want[xq == float(cols)]).any()
        if rows > 6:
            assert (xq == float(sc.ulp_up(cols))).any() and np.isnan(want[xq == float(sc.ulp_up(cols))]).all()
            assert (xq == float(sc.ulp_up(1.0))).any() and (xq == float(sc.ulp_down(cols))).any()
            inner = (xq == np.floor(xq)) & (xq > 1) & (xq < cols)
            assert inner.any()
            ii, jj = np.nonzero(inner)
            assert np.array_equal(want[ii, jj], U.astype(np.float64)[ii, xq[ii, jj].astype(int) - 1])   # an exact integer: that pixel


def test_flow_warp_cases_hit_integers_the_last_column_and_one_ulp_past():
    for name, U, V in sc.flow_warp_cases():
        rows, cols = U.shape
        X, Y = ms.flow_coords(U, V)
        assert (X[0] == np.floor(X[0])).all() and (X[0] >= 1).all() and (X[0] <= cols).all()
        assert (X[1] == F32(cols)).all()
        assert (X[2] == sc.ulp_up(cols)).any() and (X[3] == sc.ulp_down(1.0)).any()
        assert (Y[:, 0] == np.floor(Y[:, 0])).all() and (Y[:, 0] >= 1).all() and (Y[:, 0] <= rows).all()
        assert (Y[:, 1] == F32(rows)).all() and (Y[:, 2] == sc.ulp_up(rows)).any() and (Y[:, 3] == sc.ulp_down(1.0)).any()
        assert np.isnan(X).any() and np.isinf(Y).any()
