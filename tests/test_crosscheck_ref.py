"""CPU: the restatement of the cross-checks (crosscheck_ref.py) pinned independently of the library.

tests/test_gpu_crosscheck.py compares the GPU with the restatement bit for bit; here the restatement itself is held against the
statement of the symmetric driver's warp (oracle/matlab_side.sym_warp_flow), against scipy's linear map_coordinates, and against
answers known in closed form.  The seeded cases are checked to exercise both branches of `kept`."""
import math

import numpy as np
import pytest

import crosscheck_cases as cc
import crosscheck_ref as cr
from stage_edge_cases import matlab_side

F32, F64 = np.float32, np.float64


def _same_bits64(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.uint64), b[~np.isnan(b)].view(np.uint64))


@pytest.mark.parametrize("kind", cc.DISP_KINDS)
@pytest.mark.parametrize("shape", cc.DISP_SHAPES, ids=cc.shape_id)
def test_warped_disparity_is_the_symmetric_drivers_warp(shape, kind):
    ms = matlab_side()
    D0, D1, _ = cc.disp_case(shape, kind)
    with np.errstate(invalid="ignore"):
        want = ms.sym_warp_flow(D1, D0)
    assert _same_bits64(cr.warp_x(D1, D0), want)


@pytest.mark.parametrize("shape", [s for s in cc.FLOW_SHAPES if s[0] * s[1] > 4], ids=cc.shape_id)
def test_sample_agrees_with_map_coordinates(shape):
    """Two evaluation orders of a four-term float64 sum of products: 1e-12 of the field's amplitude."""
    from scipy.ndimage import map_coordinates

    Uf, Vf, Ub, Vb, _ = cc.flow_case(shape, "normal")
    rows, cols = shape
    xq = np.arange(1, cols + 1, dtype=F64)[None, :] + Uf.astype(F64)
    yq = np.arange(1, rows + 1, dtype=F64)[:, None] + Vf.astype(F64)
    ok = (xq >= 1) & (xq <= cols) & (yq >= 1) & (yq <= rows)
    assert ok.any() and (not ok.all() or rows * cols < 20)
    for A in (Ub, Vb):
        got = cr.sample_xy(A, xq, yq)
        assert np.array_equal(np.isnan(got), ~ok)
        want = map_coordinates(A.astype(F64), [yq[ok] - 1.0, xq[ok] - 1.0], order=1, mode="nearest")
        assert np.max(np.abs(got[ok] - want)) <= 1e-12 * float(np.max(np.abs(A)))


def test_sample_on_the_grid_and_on_the_last_lines():
    A = np.arange(12, dtype=F32).reshape(3, 4)
    x, y = np.meshgrid(np.arange(1.0, 5.0), np.arange(1.0, 4.0))
    assert np.array_equal(cr.sample_xy(A, x, y), A.astype(F64))            # integer queries, the last row and column among them
    assert cr.sample_xy(A, np.array([[2.5]]), np.array([[1.0]]))[0, 0] == 1.5
    assert cr.sample_xy(A, np.array([[4.0]]), np.array([[2.5]]))[0, 0] == 9.0   # (7 + 11) / 2 on the last column
    for xq, yq in ((0.999, 1.0), (4.001, 1.0), (1.0, 0.999), (1.0, 3.001), (np.nan, 1.0), (1.0, np.inf)):
        assert math.isnan(cr.sample_xy(A, np.array([[xq]]), np.array([[yq]]))[0, 0])


@pytest.mark.parametrize("d", [-3, -1, 0, 2, 5])
def test_constant_integer_disparity_against_its_negative(d):
    """r == 0 exactly: kept even at tol = 0, and exactly |d| columns look outside the other view."""
    rows, cols = 5, 17
    D0 = np.full((rows, cols), d, F32)
    D1 = np.full((rows, cols), -d, F32)
    out = cr.disp_crosscheck(D0, D1, 0.0)
    inside = out["defined_mask"]
    assert np.all(out["r"][inside] == 0.0) and np.array_equal(out["kept_mask"], inside)
    gone = np.flatnonzero(~inside.all(axis=0))
    assert len(gone) == abs(d) and np.array_equal(inside.any(axis=0), inside.all(axis=0))
    assert list(gone) == (list(range(cols - d, cols)) if d > 0 else list(range(0, -d)))
    assert out["kept"] == out["defined"] == rows * (cols - abs(d)) and out["mean"] == 0.0 and out["max"] == 0.0
    assert np.array_equal(np.isnan(out["sparse"]), ~inside) and np.all(out["sparse"][inside] == d)
    assert np.array_equal(out["mask"], inside.astype(F32))


def test_a_band_that_disagrees_is_lost_and_nothing_else():
    rows, cols = 9, 40
    D0 = np.full((rows, cols), 2.0, F32)
    D1 = np.full((rows, cols), -2.0, F32)
    D0[:, 10:15] = 5.0          # these look 5 to the right and find -2 there: r = 3
    out = cr.disp_crosscheck(D0, D1, 1.0)
    want = np.ones((rows, cols), bool)
    want[:, 10:15] = False      # the band
    want[:, cols - 2:] = False  # the two columns that look outside
    assert np.array_equal(out["kept_mask"], want)
    assert np.all(out["r"][:, 10:15] == 3.0) and out["max"] == 3.0
    assert out["defined"] == rows * (cols - 2) and out["kept"] == rows * (cols - 2 - 5)
    assert abs(out["mean"] - 15.0 * rows / out["defined"]) <= 1e-15


def test_zero_weight_tap_propagates_its_nan():
    D0 = np.zeros((1, 4), F32)
    D1 = np.array([[1.0, np.nan, 3.0, 4.0]], F32)
    out = cr.disp_crosscheck(D0, D1, np.inf)
    # pixel 0 samples column 0 with weight 1 and column 1 (NaN) with weight 0: 1 * 1 + NaN * 0 is NaN
    assert list(out["defined_mask"][0]) == [False, False, True, True]
    assert out["kept"] == 2 and out["max"] == 4.0 and out["mean"] == 3.5
    assert np.isnan(out["diff"][0, 0]) and np.isnan(out["sparse"][0, 1])


def test_negative_zero_survives_in_the_sparse_map():
    D0 = np.array([[-0.0, 0.0, -0.0]], F32)
    D1 = np.zeros((1, 3), F32)
    out = cr.disp_crosscheck(D0, D1, 0.0)
    assert out["kept"] == 3 and list(np.signbit(out["sparse"][0])) == [True, False, True]


def test_flow_criterion_by_hand():
    """A forward flow of (1, 0) everywhere against a backward flow of (-1 + d, 0): e = d^2, lim = a (1 + (1 - d)^2) + b."""
    rows, cols = 4, 6
    Uf, Vf = np.ones((rows, cols), F32), np.zeros((rows, cols), F32)
    Vb = np.zeros((rows, cols), F32)
    for d, a, b, keep in ((0.0, 0.0, 0.0, True), (0.5, 0.0, 0.25, True), (0.5, 0.0, 0.2, False), (0.5, 0.01, 0.5, True),
                          (2.0, 0.5, 2.0, False), (2.0, 1.0, 2.0, True)):
        Ub = np.full((rows, cols), -1.0 + d, F32)
        out = cr.flow_crosscheck(Uf, Vf, Ub, Vb, a, b)
        inside = np.ones((rows, cols), bool)
        inside[:, -1] = False   # the last column looks one pixel outside
        assert np.array_equal(out["defined_mask"], inside)
        assert np.all(out["err64"][inside] == d) and np.isnan(out["err"][:, -1]).all()
        assert np.array_equal(out["kept_mask"], inside & keep), (d, a, b)
        assert out["defined"] == rows * (cols - 1) and out["kept"] == (out["defined"] if keep else 0)
        assert out["max"] == d and abs(out["mean"] - d) <= 1e-15


def test_nothing_defined_gives_nan_statistics():
    D = np.full((3, 4), np.nan, F32)
    out = cr.disp_crosscheck(D, D, 1.0)
    assert out["kept"] == 0 and out["defined"] == 0 and math.isnan(out["mean"]) and math.isnan(out["max"])
    out = cr.flow_crosscheck(D, D, D, D, 0.01, 0.5)
    assert out["kept"] == 0 and out["defined"] == 0 and math.isnan(out["mean"]) and math.isnan(out["max"])
    assert np.all(out["mask"] == 0) and np.isnan(out["err"]).all()


def test_normal_cases_take_both_branches():
    """Each 'normal' case that is large enough keeps between 20 % and 80 % of its pixels.  Computed on the CPU for these seeds:
    disparity with tol = 2: 0.59 / 0.56 / 0.56 at 1x300 / 37x53 / 270x480; flow with a = 0.5, b = 2: 0.34 / 0.39 at 37x53 / 270x480."""
    seen = 0
    for shape in cc.DISP_SHAPES:
        if cc.disp_is_big(shape):
            D0, D1, tols = cc.disp_case(shape, "normal")
            share = cr.disp_crosscheck(D0, D1, tols[0])["kept"] / D0.size
            print("disparity %s tol %g: kept %.2f" % (shape, tols[0], share))
            assert tols[0] == 2.0 and 0.2 <= share <= 0.8
            seen += 1
    for shape in cc.FLOW_SHAPES:
        if cc.flow_is_big(shape):
            Uf, Vf, Ub, Vb, ab = cc.flow_case(shape, "normal")
            share = cr.flow_crosscheck(Uf, Vf, Ub, Vb, *ab[0])["kept"] / Uf.size
            print("flow %s a %g b %g: kept %.2f" % (shape, ab[0][0], ab[0][1], share))
            assert ab[0] == (0.5, 2.0) and 0.2 <= share <= 0.8
            seen += 1
    assert seen == 5


def test_every_tiny_case_keeps_a_query_in_range():
    for shape in cc.DISP_SHAPES:
        D0, D1, tols = cc.disp_case(shape, "normal")
        assert cr.disp_crosscheck(D0, D1, tols[0])["defined"] > 0, shape
    for shape in cc.FLOW_SHAPES:
        Uf, Vf, Ub, Vb, ab = cc.flow_case(shape, "normal")
        assert cr.flow_crosscheck(Uf, Vf, Ub, Vb, *ab[0])["defined"] > 0, shape


def test_edge_cases_reach_the_last_lines_and_one_ulp_outside():
    """The 'edges' fields: queries exactly on column ncols / row nrows (s = 1, t = 1) and on column / row 1 are in range, those one
    float32 ulp outside are not (where that ulp survives the addition in double)."""
    D0, D1, _ = cc.disp_case((37, 53), "edges")
    xq = np.arange(1, 54, dtype=F64)[None, :] + D0.astype(F64)
    assert (xq == 53.0).sum() > 300 and (xq == 1.0).sum() > 300 and (xq > 53.0).sum() > 300 and (xq < 1.0).sum() > 300
    assert np.array_equal(cr.disp_crosscheck(D0, D1, np.inf)["defined_mask"], (xq >= 1.0) & (xq <= 53.0))
    Uf, Vf, Ub, Vb, _ = cc.flow_case((37, 53), "edges")
    yq = np.arange(1, 38, dtype=F64)[:, None] + Vf.astype(F64)
    xq = np.arange(1, 54, dtype=F64)[None, :] + Uf.astype(F64)
    for xs in (xq == 53.0, xq == 1.0, xq > 53.0, xq < 1.0):
        for ys in (yq == 37.0, yq == 1.0, yq > 37.0, yq < 1.0):
            assert (xs & ys).sum() > 50
