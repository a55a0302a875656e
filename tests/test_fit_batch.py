"""CPU: the batched masked fit (pdeip_surface_fit_masked_batch_dev) at the boundary -- exported, bound, and every refusal of
include/pdeip.h fired before any HIP call (there is no GPU here: a refusal that came after one would report PDEIP_ERR_DEVICE) --
its restatement (ransac_batch_ref.surface_fit_masked_batch) against the loop it restates, and the conditions on the inputs the GPU tests
use (fit_batch_cases.py)."""
import ctypes
import math

import numpy as np
import pytest

import fit_batch_cases as fc
import ransac_ref as ref
from test_capi_symbols import declared_symbols

F32 = np.float32
NAME = "pdeip_surface_fit_masked_batch_dev"
PTR = 64  # a non-NULL address that a refused call must not touch


def test_header_declares_and_library_exports_the_entry(pdeip):
    lib = ctypes.CDLL(pdeip.capi.LIB_PATH)
    assert NAME in declared_symbols() and hasattr(lib, NAME) and NAME in pdeip.capi.SIGNATURES
    assert len(pdeip.capi.SIGNATURES[NAME]) == 16


def _refused(capi, PHI=PTR, D=PTR, nrows=8, ncols=8, S=2, order=1, M_in=None, thr=0.5, mss=0.5, iter=3, M_out=PTR, dist=None):
    with pytest.raises(capi.PdeipError) as e:
        capi.call(NAME, None, PHI, D, nrows, ncols, S, order, M_in, thr, mss, iter, ctypes.c_ulonglong(1), ctypes.c_ulonglong(65536), M_out,
                  dist, None)
    assert e.value.code == capi.PDEIP_ERR_ARG, str(e.value)
    assert NAME in str(e.value), str(e.value)
    return str(e.value)


def test_refusals_come_before_any_hip_call(pdeip):
    capi = pdeip.capi
    assert "'PHI' is NULL" in _refused(capi, PHI=None)
    assert "'D' is NULL" in _refused(capi, D=None)
    assert "'M_out' is NULL" in _refused(capi, M_out=None)
    for S in (0, -1, 65536):
        assert "1 .. 65535" in _refused(capi, S=S)
    for order in (0, 3):
        assert "order must be 1 or 2" in _refused(capi, order=order)
    assert "must not be empty" in _refused(capi, nrows=0)
    assert "must not be empty" in _refused(capi, ncols=-2)
    for bad in (math.nan, math.inf, -math.inf):
        assert "err_thr must be finite" in _refused(capi, thr=bad)
        assert "min_set_size must be finite" in _refused(capi, mss=bad)
    for it in (0, -2):
        assert "nothing to return" in _refused(capi, iter=it)
    assert "too large" in _refused(capi, iter=32 * 65535)          # the iter bound of the single call
    assert "too large" in _refused(capi, nrows=1 << 15, ncols=1 << 15)
    assert "2^31-1 elements" in _refused(capi, nrows=4096, ncols=4096, S=128)   # S*nrows*ncols = 2^31
    assert "2^31-1 elements" in _refused(capi, nrows=64, ncols=64, S=65535, iter=2000)  # the models and partials alone
    assert "must not alias" in _refused(capi, dist=PTR)


# ---- the restatement ------------------------------------------------------------------------------------------------------------

def _same(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", ["s3_37x53_o2_alias", "s3_37x53_o2_wrap", "s3_37x53_o1_stride0"])
def test_restatement_is_the_loop_over_single_fits(name):
    PHI, D, M_in, c, (res, M, dist, ndata) = fc.case(name)
    assert M.shape == ((3 if c["order"] == 1 else 6), PHI.shape[2]) and dist.shape == PHI.shape and ndata.shape == (PHI.shape[2],)
    for s in range(PHI.shape[2]):
        seed = (c["seed"] + c["stride"] * s) % 2 ** 64
        r, m, d, n = ref.surface_fit_masked(PHI[:, :, s], D, c["order"], None if M_in is None else M_in[:, s], fc.ERR_THR, fc.MIN_SET, c["iter"], seed=seed)
        assert _same(m, M[:, s]) and _same(d, dist[:, :, s]) and n == ndata[s]
        assert (r is None) == (res[s] is None)
        if r is not None:
            assert r["winner"] == res[s]["winner"] and np.array_equal(r["inliers"], res[s]["inliers"])
    if name == "s3_37x53_o2_wrap":
        assert c["seed"] + c["stride"] * 2 >= 2 ** 64  # the sum does wrap


# ---- conditions on the GPU tests' inputs ----------------------------------------------------------------------------------------

def test_every_gpu_case_has_a_safe_decision_margin():
    """Two summation orders of n float64 terms differ by at most 2(n-1)*2^-53 relative (5e-12 at n = 33792): every `sum < best_sum`
    the restatement decides between models that are not bit-identical is decided by more than 1e-9 relative.  Two sums over NO
    inliers are both the empty sum, 0 in any order: such a pair (a mask of one pixel, where every hypothesis is singular, is one) has
    nothing to decide and is passed over."""
    worst = 1.0
    for name, r, M_in in fc.all_margins():
        for h, s, best_sum, best in r["margins"]:
            if best is None:
                continue  # against the initial FLT_MAX
            holder = M_in if best == -1 else r["models"][best]
            if _same(holder, r["models"][h]) and (best == -1 or r["singular"][best] == r["singular"][h]):
                continue
            if r["inliers"][1 + h] == 0 and r["inliers"][1 + best] == 0:
                assert s == 0.0 and best_sum == 0.0
                continue
            top = max(abs(s), abs(best_sum))
            rel = abs(s - best_sum) / top if top > 0 else 0.0
            assert rel > 1e-9, (name, h, s, best_sum)
            worst = min(worst, rel)
    print("smallest decision margin: %.3g relative" % worst)


def test_cases_take_the_paths_they_are_meant_to():
    sizes = {}
    for name, c in fc.CASES.items():
        PHI, D, M_in, _, (res, M, dist, ndata) = fc.case(name)
        S = PHI.shape[2]
        sizes.setdefault(c["shape"], set()).add(S)
        assert S <= 3 or c["shape"] != (176, 192)
        by = dict(zip(c["masks"], ndata))
        npix = PHI.shape[0] * PHI.shape[1]
        for m, want in (("full", npix), ("empty", 0), ("one", 1), ("b256", 256), ("b257", 257), ("stripe_small", 2 * PHI.shape[0]),
                        ("negzero", 2 * PHI.shape[0])):
            assert m not in by or by[m] == want, (name, m)
        for s in range(S):
            if ndata[s] == 0:
                assert res[s] is None
                assert (np.isnan(M[:, s]).all() if M_in is None else _same(M[:, s], M_in[:, s])), name
        assert all(a != b for a, b in zip(c["masks"], c["masks"][1:])), name  # neighbouring segments differ
        if S == 17:  # every large set holds an empty mask, a mask of one pixel and a pair of identical planes
            assert 0 in ndata and 1 in ndata
            assert _same(PHI[:, :, 4], PHI[:, :, 11]) and ndata[4] > 256
            assert ndata.max() > 20 * ndata[ndata > 1].min()  # very different counts: most score blocks of a small segment exit early
    assert sizes[(37, 53)] >= {1, 3, 17} and sizes[(64, 80)] >= {3, 17} and sizes[(176, 192)] <= {2, 3}
    its = {c["iter"] for c in fc.CASES.values()}
    assert its >= {0, 10, 100}
    assert {(c["given"], c["alias"]) for c in fc.CASES.values()} >= {(True, True), (True, False), (False, False)}
    assert {c["order"] for c in fc.CASES.values() if c["iter"] == 100} == {1, 2}
    PHI, D, _, _, (res, M, dist, _) = fc.case("s3_37x53_o1_nan_d")
    assert np.isnan(D).any() and np.isnan(dist).any() and not np.isnan(M).any()
    assert np.isnan(fc.case("s17_37x53_o2")[0][:, :, 9]).any() and np.signbit(fc.case("s17_37x53_o2")[0][:, :, 10][fc.case("s17_37x53_o2")[0][:, :, 10] == 0]).any()
    # identical planes with stride 0: identical columns and planes; with the default stride the draws differ
    _, _, _, _, (_, M, dist, _) = fc.case("s3_37x53_o1_stride0")
    assert _same(M[:, 0], M[:, 2]) and _same(dist[:, :, 0], dist[:, :, 2])
    _, _, _, _, (res, M, _, _) = fc.case("s17_37x53_o2")
    assert not np.array_equal(res[4]["models"], res[11]["models"])
