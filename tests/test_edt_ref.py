"""CPU: the NumPy restatement of the distance transform (tests/edt_ref.py) is pinned -- its separable form against the brute-force
minimum of (d2, idx) over all features, its distances against SciPy where SciPy imports, the tie rule on a case where a third of the
pixels tie -- and what the nearest-source fill buys on the interpolation scene is asserted.  The GPU half is tests/test_gpu_edt.py."""
import numpy as np
import pytest

import edt_cases as ec
import edt_ref
import inpaint_cases
import interp_cases

F32 = np.float32


def _same(a, b):
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))


@pytest.mark.parametrize("case", ec.cases(), ids=ec.case_id)
def test_separable_equals_brute_force(case):
    """Every mask and its complement, every max_dist: the box search of the separable form loses nothing and keeps the tie rule."""
    shape, kind = case
    M = ec.mask(shape, kind)
    for complement in (False, True):
        A = np.where(M != complement, F32(1.0), F32(0.0))
        d2, idx, _ = edt_ref.edt_brute(A, edt_ref.POSITIVE, 0)      # the minimum over all features once; max_dist acts on its result
        for R in ec.MAX_DISTS:
            assert _same(ec.want(shape, kind, complement, R), edt_ref.limit(d2, idx, R)), (complement, R)


@pytest.mark.parametrize("case", ec.cases(), ids=ec.case_id)
def test_planes_dress_their_masks(case):
    """plane() under its mode has exactly mask()'s features, the _NOT twin the complement: the predicates on NaN, +-Inf, +-0, subnormals."""
    shape, kind = case
    M = ec.mask(shape, kind)
    for mode in ec.BASE_MODES:
        A = ec.plane(shape, kind, mode)
        assert np.array_equal(edt_ref.features(A, mode), M), mode
        assert np.array_equal(edt_ref.features(A, mode | 4), ~M), mode
    specials = np.array([-0.0, np.nan, np.inf, -np.inf, 1e-40, -1e-40], F32)
    assert np.array_equal(edt_ref.features(specials, edt_ref.POSITIVE), [False, False, True, False, True, False])
    assert np.array_equal(edt_ref.features(specials, edt_ref.NONNEG), [True, False, True, False, True, False])
    assert np.array_equal(edt_ref.features(specials, edt_ref.NOT_NAN), [True, False, True, True, True, True])


def test_frames_are_independent():
    for shape, kinds in ec.FRAME_CASES:
        A = ec.frames(shape, kinds, edt_ref.POSITIVE)
        got = edt_ref.edt(A, edt_ref.POSITIVE, 3)
        assert _same(got, ec.want_frames(shape, kinds, False, 3))
        assert got[0].shape == shape + (len(kinds),)


@pytest.mark.parametrize("case", ec.cases(), ids=ec.case_id)
def test_distances_equal_scipy(case):
    """Distances only: SciPy's indices follow another tie rule.  (SciPy has no answer for a mask without a feature.)"""
    ndimage = pytest.importorskip("scipy.ndimage")
    shape, kind = case
    M = ec.mask(shape, kind)
    d2, idx, dist = ec.want(shape, kind, False, 0)
    if not M.any():
        assert (d2 == edt_ref.I32_MAX).all() and (idx == -1).all() and np.isinf(dist).all()
        return
    assert np.array_equal(np.sqrt(d2.astype(np.float64)), ndimage.distance_transform_edt(~M))


def test_the_tie_rule_is_exercised():
    """On the checkerboard more than a third of the pixels have several nearest features, and the one reported is the lowest index of
    them -- the brute force says so by construction, the separable form agrees (above); here the count and one pixel by hand."""
    shape, kind = ec.TIE_CASE
    A = ec.plane(shape, kind, edt_ref.POSITIVE)
    ties = edt_ref.tie_count(A)
    n = shape[0] * shape[1]
    print("tied pixels on %s %s: %d of %d" % (ec.shape_id(shape), kind, ties, n))
    assert 3 * ties > n
    d2, idx, _ = ec.want(shape, kind, False, 0)
    # pixel (1, 2) is off the board; its four neighbours (0,2), (2,2), (1,1), (1,3) are on it: the lowest index is column 1
    assert d2[1, 2] == 1 and idx[1, 2] == 1 * shape[0] + 1
    # the same from the left column: (1, 0) has (0,0), (2,0), (1,1): column 0, the upper row
    assert d2[1, 0] == 1 and idx[1, 0] == 0
    pair = ec.mask((37, 53), "pair")
    assert edt_ref.tie_count(np.where(pair, F32(1), F32(0))) == 37       # the whole bisector column
    assert np.all(ec.want((37, 53), "pair", False, 0)[1][:, 26] == 18)  # ... goes to the left feature, (18, 0)


def test_signed_distance_by_hand():
    A = np.array([[-1, -1, -1, -1, -1], [-1, 2, -0.0, 5, -1], [-1, -1, np.nan, -1, -1]], F32)
    S = edt_ref.signed_distance(A)
    assert S.dtype == F32 and np.all(np.abs(S) >= 0.5)
    assert np.array_equal(np.signbit(S), ~edt_ref.features(A, edt_ref.NONNEG))
    assert np.array_equal(S[1], F32([-0.5, 0.5, 0.5, 0.5, -0.5]))
    assert S[2, 2] == F32(-0.5) and S[0, 0] == -(F32(np.sqrt(2.0)) - F32(0.5))
    assert np.all(edt_ref.signed_distance(np.ones((3, 4), F32)) == np.inf)
    assert np.all(edt_ref.signed_distance(-np.ones((3, 4), F32)) == -np.inf)
    assert np.all(edt_ref.signed_distance(np.ones((3, 4), F32), 2) == F32(2.5))
    far = np.full((1, 9), -1, F32)
    far[0, 0] = 1
    assert np.array_equal(edt_ref.signed_distance(far, 3)[0], F32([0.5, -0.5, -1.5, -2.5, -3.5, -3.5, -3.5, -3.5, -3.5]))


def test_nearest_fill_by_hand():
    nan = np.nan
    D = np.array([[nan, -0.0, nan, nan, nan, 7.0], [nan, nan, nan, nan, nan, nan]], F32)
    out, filled, dist = edt_ref.nearest_fill(D)
    assert np.array_equal(out[0], F32([-0.0, -0.0, -0.0, -0.0, 7.0, 7.0])) and np.signbit(out[0, :4]).all()
    assert np.array_equal(filled, np.isnan(D).astype(F32)) and dist[1, 3] == F32(np.sqrt(5.0))   # (1,3): (0,1) wins the tie with (0,5)
    assert out[1, 3] == 0 and np.signbit(out[1, 3])
    out, filled, _ = edt_ref.nearest_fill(D, 1)
    assert np.isnan(out[0, 3]) and filled[0, 3] == 0 and out[1, 1] == 0 and filled[1, 1] == 1 and np.isnan(out[1, 0])
    out, filled, dist = edt_ref.nearest_fill(np.full((2, 3), nan, F32))
    assert np.isnan(out).all() and not filled.any() and np.isinf(dist).all()


def test_interpolation_quality_with_the_nearest_fill():
    """The scene of interp_cases: the chain with the nearest-source fill beats the average of the two frames with and without the
    backward flow, and the backward flow does not hurt.  (Measured when this was written: 0.0156 and 0.0050 against 0.0691.)"""
    I0, I1, Imid, Uf, Vf, Ub, Vb, valid = interp_cases.scene()
    average = interp_cases.rms((I0.astype(np.float64) + I1) / 2, Imid, valid)
    one = interp_cases.rms(edt_ref.flow_interpolate_nearest(I0, I1, Uf, Vf)[0], Imid, valid)
    two = interp_cases.rms(edt_ref.flow_interpolate_nearest(I0, I1, Uf, Vf, Ub, Vb)[0], Imid, valid)
    print("rms against the true middle frame: average %.4f, nearest chain %.4f, with the backward flow %.4f" % (average, one, two))
    assert one < average and two < average
    assert two <= one


def test_stereo_band_limitation_is_documented():
    """Not asserted: on an occlusion band the nearest neighbour is the foreground, so the cheap fill is worse than the mean there
    (3.45 px against 3.11 over the holes; TV inpainting: 1.20)."""
    truth, sparse, _, _ = inpaint_cases.scene()
    hole = np.isnan(sparse)
    out, _, _ = edt_ref.nearest_fill(sparse)
    mean = np.where(hole, np.nanmean(sparse.astype(np.float64)), sparse)
    print("stereo scene, rms over the %d holes: nearest fill %.2f px, mean fill %.2f px" % (
        int(hole.sum()), inpaint_cases.rms(out, truth, hole), inpaint_cases.rms(mean, truth, hole)))
    assert np.array_equal(out[~hole], sparse[~hole]) and not np.isnan(out).any()
