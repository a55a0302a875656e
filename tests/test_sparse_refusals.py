"""CPU: the sparse driver's calls refuse what include/pdeip.h says they refuse BEFORE any HIP call -- there is no GPU here, so a
refusal that came after one would report PDEIP_ERR_DEVICE instead.  The data pointers are never dereferenced."""
import ctypes
import math

import pytest

PTR = 64  # a non-NULL address that a refused call must not touch
CSET = (ctypes.c_double * 3)(0.1, 0.4, 0.7)


def _refused(capi, code, name, *args):
    with pytest.raises(capi.PdeipError) as e:
        capi.call(name, *args)
    assert e.value.code == code, str(e.value)
    return str(e.value)


def test_nanmedfilt2_refusals(pdeip):
    capi = pdeip.capi
    ARG = capi.PDEIP_ERR_ARG
    for name, lead in (("pdeip_nanmedfilt2_dev", (None,)), ("pdeip_nanmedfilt2", ())):
        assert "NULL" in _refused(capi, ARG, name, *lead, None, 4, 4, 1, PTR + 4096)
        assert "NULL" in _refused(capi, ARG, name, *lead, PTR, 4, 4, 1, None)
        for bad in (0, -3):
            assert "1x1" in _refused(capi, ARG, name, *lead, PTR, bad, 4, 1, PTR + 4096)
            assert "1x1" in _refused(capi, ARG, name, *lead, PTR, 4, bad, 1, PTR + 4096)
            assert "frames" in _refused(capi, ARG, name, *lead, PTR, 4, 4, bad, PTR + 4096)
        assert "INT_MAX" in _refused(capi, ARG, name, *lead, PTR, 46341, 46341, 1, PTR + 4096)
        assert "alias" in _refused(capi, ARG, name, *lead, PTR, 4, 4, 1, PTR)
        assert "columns" in _refused(capi, capi.PDEIP_ERR_UNSUPPORTED, name, *lead, PTR, 4, 65536, 1, PTR + 4096)


def _pyramid(capi, D=PTR, nrows=8, ncols=8, scl_factor=0.75, pyr_scl=0.55, cap=8, K=True, sizes=True, out=PTR + 4096, code=None):
    k = ctypes.c_int(-7)
    sz = (ctypes.c_int * 16)(*([-7] * 16))
    msg = _refused(capi, code or capi.PDEIP_ERR_ARG, "pdeip_sparse_pyramid", D, nrows, ncols, scl_factor, pyr_scl, cap,
                   ctypes.addressof(k) if K else None, ctypes.addressof(sz) if sizes else None, out)
    assert k.value == -7 and all(v == -7 for v in sz)
    return msg


def test_sparse_pyramid_refusals_and_sizes(pdeip):
    capi = pdeip.capi
    assert "NULL" in _pyramid(capi, K=False)
    assert "NULL" in _pyramid(capi, sizes=False)
    assert "NULL" in _pyramid(capi, D=None)
    assert "3x3" in _pyramid(capi, nrows=2)
    assert "3x3" in _pyramid(capi, ncols=2)
    assert "INT_MAX" in _pyramid(capi, nrows=46341, ncols=46341)
    for bad in (0.0, 1.0, 1.5, -0.5, math.nan):
        assert "scl_factor" in _pyramid(capi, scl_factor=bad)
    for bad in (0.0, -0.2, math.inf, math.nan):
        assert "pyr_scl" in _pyramid(capi, pyr_scl=bad)
    assert "scales_cap" in _pyramid(capi, cap=0)
    assert "scales_cap" in _pyramid(capi, nrows=60, ncols=80, cap=2)  # K = 3
    assert "columns" in _pyramid(capi, nrows=8, ncols=65536, code=capi.PDEIP_ERR_UNSUPPORTED)
    # out == NULL: the sizes only, without any HIP call (so it succeeds without a GPU) and without reading D
    k = ctypes.c_int(0)
    sz = (ctypes.c_int * 16)()
    capi.call("pdeip_sparse_pyramid", None, 60, 80, 0.75, 0.55, 8, ctypes.addressof(k), ctypes.addressof(sz), None)
    assert k.value == 3 and list(sz[:6]) == [60, 80, 45, 60, 34, 45]


def _seeds(capi, D=PTR, nrows=8, ncols=8, order=1, sigmaLim=0.7, cset=CSET, n_cset=3, iterations=3, seeds=2, scl_factor=0.75, pyr_scl=0.55,
           S_out=True, PHI_out=PTR + 4096, surf_out=PTR):
    s_out = ctypes.c_int(-7)
    msg = _refused(capi, capi.PDEIP_ERR_ARG, "pdeip_generate_seeds_sparse", D, None, nrows, ncols, order, sigmaLim,
                   None if cset is None else ctypes.addressof(cset), n_cset, iterations, seeds, scl_factor, pyr_scl, ctypes.c_ulonglong(0), None,
                   None, None, ctypes.addressof(s_out) if S_out else None, PHI_out, surf_out)
    assert s_out.value == -7 and "pdeip_generate_seeds_sparse" in msg
    return msg


def test_generate_seeds_sparse_refusals(pdeip):
    capi = pdeip.capi
    assert "NULL" in _seeds(capi, D=None)
    assert "NULL" in _seeds(capi, S_out=False)
    assert "NULL" in _seeds(capi, PHI_out=None)
    assert "NULL" in _seeds(capi, surf_out=None)
    assert "3x3" in _seeds(capi, nrows=2)
    assert "3x3" in _seeds(capi, ncols=2)
    assert "seeds" in _seeds(capi, seeds=0)
    assert "too large" in _seeds(capi, nrows=20000, ncols=20000)
    assert "iterations" in _seeds(capi, iterations=-1)
    for order in (0, 3):
        assert "order" in _seeds(capi, order=order)
    for bad in (math.nan, math.inf, 0.0, -1.0):
        assert "sigmaLim" in _seeds(capi, sigmaLim=bad)
    assert "cset_vect" in _seeds(capi, n_cset=0)
    assert "cset_vect" in _seeds(capi, cset=None)
    assert "cset_vect[1]" in _seeds(capi, cset=(ctypes.c_double * 3)(0.1, math.nan, 0.7))
    for bad in (0.0, 1.0, math.nan):
        assert "scl_factor" in _seeds(capi, scl_factor=bad)
    for bad in (0.0, math.inf, math.nan):
        assert "pyr_scl" in _seeds(capi, pyr_scl=bad)


def _rc(capi, D=PTR, PHI=PTR + 4096, nrows=8, ncols=8, S=2, order=1, strategy=2, sigmaLim=1.0, cset=0.7, iterations=3, srem_thr=0.002,
        scl_factor=0.75, rc_scl=0.55, S_out=True, PHI_out=PTR + 8192, surf_out=PTR, kept=PTR):
    s_out = ctypes.c_int(-7)
    msg = _refused(capi, capi.PDEIP_ERR_ARG, "pdeip_region_competition_sparse", D, PHI, nrows, ncols, S, order, strategy, sigmaLim, cset, iterations,
                   srem_thr, scl_factor, rc_scl, ctypes.c_ulonglong(0), None, ctypes.addressof(s_out) if S_out else None, PHI_out, surf_out, kept)
    assert s_out.value == -7 and "pdeip_region_competition_sparse" in msg
    return msg


def test_region_competition_sparse_refusals(pdeip):
    capi = pdeip.capi
    assert "NULL" in _rc(capi, D=None)
    assert "NULL" in _rc(capi, PHI=None)
    assert "NULL" in _rc(capi, S_out=False)
    assert "NULL" in _rc(capi, PHI_out=None)
    assert "NULL" in _rc(capi, surf_out=None)
    assert "NULL" in _rc(capi, kept=None)
    assert "segments" in _rc(capi, S=0)
    assert "order" in _rc(capi, order=3)
    assert "strategy" in _rc(capi, strategy=5)
    for bad in (math.nan, math.inf, 0.0):
        assert "minCOV" in _rc(capi, sigmaLim=bad)
    assert "iterations" in _rc(capi, iterations=-1)
    assert "finite" in _rc(capi, srem_thr=math.inf)
    assert "scl_factor" in _rc(capi, scl_factor=1.0)
    assert "rc_scl" in _rc(capi, rc_scl=0.0)
    assert "3x3" in _rc(capi, nrows=2)


class _Prm(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in ("srem_thr", "scl_factor", "gen_scl", "rc_scl", "ransac_min_cset", "ransac_max_cset")] + \
               [(k, ctypes.c_int) for k in ("polyorder", "seeds", "ransac_cset_cycles")]


def _driver(capi, nrows=8, ncols=8, PHIin=None, S_in=0, Din=PTR, **over):
    vals = dict(srem_thr=math.nan, scl_factor=math.nan, gen_scl=math.nan, rc_scl=math.nan, ransac_min_cset=math.nan, ransac_max_cset=math.nan,
                polyorder=0, seeds=0, ransac_cset_cycles=0)
    vals.update(over)
    prm = _Prm(*[vals[k] for k, _ in _Prm._fields_])
    s_out = ctypes.c_int(-7)
    msg = _refused(capi, capi.PDEIP_ERR_ARG, "pdeip_disp_segmentation_sparse", Din, nrows, ncols, PHIin, S_in, None, ctypes.addressof(prm),
                   ctypes.c_ulonglong(0), ctypes.addressof(s_out), PTR + 4096, PTR, PTR)
    assert s_out.value == -7 and "pdeip_disp_segmentation_sparse" in msg
    return msg


def test_disp_segmentation_sparse_refusals(pdeip):
    capi = pdeip.capi
    assert "NULL" in _driver(capi, Din=None)
    assert "3x3" in _driver(capi, nrows=2)
    assert "order" in _driver(capi, polyorder=3)
    assert "seeds" in _driver(capi, seeds=-1)
    assert "scl_factor" in _driver(capi, scl_factor=1.0)
    assert "gen_scl" in _driver(capi, gen_scl=0.0)
    assert "rc_scl" in _driver(capi, rc_scl=-1.0)
    assert "cycles" in _driver(capi, ransac_cset_cycles=-2)
    assert "finite" in _driver(capi, ransac_max_cset=math.inf)
    assert "finite" in _driver(capi, srem_thr=math.inf)
    assert "S_in" in _driver(capi, PHIin=PTR, S_in=0)
