"""CPU: the connected-component restatement (tests/ccl_ref.py) against scipy.ndimage.label on every case of tests/ccl_cases.py, what
the case list has to contain, and the refusals of the entry points, which come back before any HIP call (there is no GPU here)."""
import ctypes

import numpy as np
import pytest
from scipy import ndimage

import ccl_cases
import ccl_ref

PTR = 64  # a non-NULL address that a refused call must not touch


@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("name", ccl_cases.names())
def test_flood_fill_equals_scipy_on_the_transposed_mask(name, conn):
    """scipy numbers in C (row-major) scan order; on the transposed mask that is MATLAB's column-major order."""
    A = ccl_cases.get(name)
    L, num, areas = ccl_ref.label(A, conn)
    structure = np.ones((3, 3), int) if conn == 8 else None
    want, n = ndimage.label(ccl_ref.foreground(A).T, structure=structure)
    assert num == n
    assert np.array_equal(L, want.T)
    assert np.array_equal(areas, np.bincount(want.ravel(), minlength=n + 1)[1:])
    assert L.dtype == np.int32 and areas.dtype == np.int32


def test_case_list_contains_every_class():
    names = ccl_cases.names()
    assert len(set(names)) == len(names)
    for cls in ccl_cases.CLASSES:
        assert any(n.startswith(cls) for n in names), cls
    for shape in ((1, 1), (1, 70), (70, 1), (2, 2)):
        for kind in ("fg", "bg", "alt"):
            assert ccl_cases.get("min_%dx%d_%s" % (shape + (kind,))).shape == shape
    for shape in ccl_cases.RANDOM_SIZES:
        for d in ccl_cases.RANDOM_DENSITIES:
            assert ccl_cases.get("random_%dx%d_%02d" % (shape + (int(100 * d),))).shape == shape
    # both forms are reachable: planes the one-workgroup form admits and planes it does not
    assert any(ccl_cases.admits_small(A) for _, A in ccl_cases.cases()) and any(not ccl_cases.admits_small(A) for _, A in ccl_cases.cases())


def test_cases_are_what_they_claim():
    lab = ccl_ref.label
    chk = ccl_cases.get("checker_64x64")
    assert lab(chk, 8)[1] == 1 and lab(chk, 4)[1] == 64 * 64 // 2  # diagonal contacts only; the largest num a plane can have
    for name in ("diag_plus_130x131", "diag_minus_130x131"):
        A = ccl_cases.get(name)
        assert lab(A, 4)[1] == int((A > 0).sum())  # all singletons under 4
        assert lab(A, 8)[1] == len({(i + j if "plus" in name else i - j) for i, j in zip(*np.nonzero(A))})  # one per line under 8
    for name in ("serpentine_130x131", "spiral_130x131"):
        A = ccl_cases.get(name)
        L, num, areas = lab(A, 4)
        assert num == 1 and A[0, 0] > 0 and areas[0] > 130 * 131 // 2 - 200  # one chain, its root at one far end
        fg = A > 0
        inner = fg[1:-1, 1:-1]
        nb = fg[:-2, 1:-1].astype(int) + fg[2:, 1:-1] + fg[1:-1, :-2] + fg[1:-1, 2:]
        assert (nb[inner] <= 2).mean() > 0.97  # one pixel wide: a chain, no blobs
    for spine in ("last_row", "first_row", "last_col", "first_col"):
        assert lab(ccl_cases.get("comb_%s_130x131" % spine), 4)[1] == 1
    t = ccl_cases.get("threshold_67x130")
    assert np.isnan(t).sum() == 200 and np.isposinf(t).sum() == 200 and np.isneginf(t).sum() == 200
    assert (t == np.float32(1e-45)).sum() == 200 and (t == np.float32(-1e-45)).sum() == 200 and (t == 0).sum() == 400
    fg = ccl_ref.foreground(t)
    assert fg[np.isposinf(t)].all() and fg[t == np.float32(1e-45)].all()
    assert not fg[np.isnan(t)].any() and not fg[t == 0].any() and not fg[t == np.float32(-1e-45)].any() and not fg[np.isneginf(t)].any()
    tie = ccl_ref.label(ccl_cases.get("largest_tie_40x90"), 8)
    assert tie[1] == 3 and tie[2][0] == tie[2][2] == 30
    out, num, area = ccl_ref.largest_component(ccl_cases.get("largest_tie_40x90"), 8, 5.0, -5.0)
    assert area == 30 and out[3, 2] == 5.0 and out[20, 60] == -5.0  # the lower label wins
    last = ccl_ref.label(ccl_cases.get("largest_last_70x140"), 8)
    assert int(np.argmax(last[2])) == last[1] - 1
    assert ccl_ref.largest_component(ccl_cases.get("largest_none_70x140"))[1:] == (0, 0)


def test_random_masks_have_a_unique_largest_component():
    for shape in ccl_cases.RANDOM_SIZES[:3]:
        for d in ccl_cases.RANDOM_DENSITIES:
            for conn in (4, 8):
                areas = ccl_ref.label(ccl_cases.get("random_%dx%d_%02d" % (shape + (int(100 * d),))), conn)[2]
                assert (areas == areas.max()).sum() == 1


def _refused(capi, name, *args):
    with pytest.raises(capi.PdeipError) as e:
        capi.call(name, *args)
    assert e.value.code == capi.PDEIP_ERR_ARG, "%s: %s" % (name, e.value)
    return str(e.value)


def test_refusals_come_before_any_hip_call(pdeip):
    capi = pdeip.capi
    num = ctypes.c_int(-7)
    pn = ctypes.addressof(num)
    big = 46341  # 46341^2 > INT_MAX
    for dev in (True, False):
        s = (None,) if dev else ()
        bw = "pdeip_bwlabel_dev" if dev else "pdeip_bwlabel"
        lc = "pdeip_largest_component_dev" if dev else "pdeip_largest_component"
        assert "NULL" in _refused(capi, bw, *s, None, 8, 8, 8, PTR, pn, None, 0)
        assert "NULL" in _refused(capi, bw, *s, PTR, 8, 8, 8, None, pn, None, 0)
        assert "NULL" in _refused(capi, bw, *s, PTR, 8, 8, 8, PTR + 4096, None, None, 0)
        assert ">= 1" in _refused(capi, bw, *s, PTR, 0, 8, 8, PTR + 4096, pn, None, 0)
        assert ">= 1" in _refused(capi, bw, *s, PTR, 8, -1, 8, PTR + 4096, pn, None, 0)
        assert "INT_MAX" in _refused(capi, bw, *s, PTR, big, big, 8, PTR + 4096, pn, None, 0)
        for conn in (0, 6, 9, -8):
            assert "conn" in _refused(capi, bw, *s, PTR, 8, 8, conn, PTR + 4096, pn, None, 0)
        assert "areas_cap" in _refused(capi, bw, *s, PTR, 8, 8, 8, PTR + 4096, pn, PTR + 8192, -1)
        assert "NULL" in _refused(capi, lc, *s, None, 8, 8, 8, 1.0, 0.0, PTR, None, None)
        assert "NULL" in _refused(capi, lc, *s, PTR, 8, 8, 8, 1.0, 0.0, None, None, None)
        assert ">= 1" in _refused(capi, lc, *s, PTR, 8, 0, 8, 1.0, 0.0, PTR, None, None)
        assert "INT_MAX" in _refused(capi, lc, *s, PTR, big, big, 8, 1.0, 0.0, PTR, None, None)
        assert "conn" in _refused(capi, lc, *s, PTR, 8, 8, 5, 1.0, 0.0, PTR, None, None)
    assert num.value == -7
