"""CPU: pdeip_generate_seeds and pdeip_disp_segmentation refuse what include/pdeip.h says they refuse BEFORE any HIP call -- there is
no GPU here, so a refusal that came after one would report PDEIP_ERR_DEVICE instead.  The data pointers are never dereferenced."""
import ctypes
import math

import pytest

PTR = 64  # a non-NULL address that a refused call must not touch
CSET = (ctypes.c_double * 3)(0.1, 0.4, 0.7)


def _seeds(capi, D=PTR, nrows=8, ncols=8, order=1, sigmaLim=0.7, cset=CSET, n_cset=3, iterations=3, seeds=2, scl_factor=0.7, pyr_scl=0.4,
           S_out=True, PHI_out=PTR + 4096, surf_out=PTR):
    s_out = ctypes.c_int(-7)
    with pytest.raises(capi.PdeipError) as e:
        capi.call("pdeip_generate_seeds", D, None, nrows, ncols, order, sigmaLim, None if cset is None else ctypes.addressof(cset), n_cset,
                  iterations, seeds, scl_factor, pyr_scl, ctypes.c_ulonglong(0), None, None, None,
                  ctypes.addressof(s_out) if S_out else None, PHI_out, surf_out)
    assert e.value.code == capi.PDEIP_ERR_ARG, str(e.value)
    assert s_out.value == -7
    return str(e.value)


def test_generate_seeds_refusals(pdeip):
    capi = pdeip.capi
    assert "NULL" in _seeds(capi, D=None)
    assert "NULL" in _seeds(capi, S_out=False)
    assert "NULL" in _seeds(capi, PHI_out=None)
    assert "NULL" in _seeds(capi, surf_out=None)
    assert "3x3" in _seeds(capi, nrows=2)
    assert "3x3" in _seeds(capi, ncols=2)
    assert "seeds" in _seeds(capi, seeds=0)
    assert "seeds" in _seeds(capi, seeds=-3)
    assert "too large" in _seeds(capi, nrows=20000, ncols=20000)
    assert "iterations" in _seeds(capi, iterations=-1)
    for order in (0, 3):
        assert "order" in _seeds(capi, order=order)
    for bad in (math.nan, math.inf, 0.0, -1.0):
        assert "sigmaLim" in _seeds(capi, sigmaLim=bad)
    assert "cset_vect" in _seeds(capi, n_cset=0)
    assert "cset_vect" in _seeds(capi, cset=None)
    for bad in (math.nan, math.inf):
        assert "cset_vect[1]" in _seeds(capi, cset=(ctypes.c_double * 3)(0.1, bad, 0.7))
    for bad in (0.0, 1.0, 1.5, -0.5, math.nan):
        assert "scl_factor" in _seeds(capi, scl_factor=bad)
    for bad in (0.0, -0.2, math.inf, math.nan):
        assert "pyr_scl" in _seeds(capi, pyr_scl=bad)


class _Prm(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in ("srem_thr", "scl_factor", "gen_scl", "rc_scl", "ransac_min_cset", "ransac_max_cset")] + \
               [(k, ctypes.c_int) for k in ("polyorder", "seeds", "ransac_cset_cycles")]


def _driver(capi, nrows=8, ncols=8, PHIin=None, S_in=0, Din=PTR, **over):
    vals = dict(srem_thr=math.nan, scl_factor=math.nan, gen_scl=math.nan, rc_scl=math.nan, ransac_min_cset=math.nan, ransac_max_cset=math.nan,
                polyorder=0, seeds=0, ransac_cset_cycles=0)
    vals.update(over)
    prm = _Prm(*[vals[k] for k, _ in _Prm._fields_])
    s_out = ctypes.c_int(-7)
    with pytest.raises(capi.PdeipError) as e:
        capi.call("pdeip_disp_segmentation", Din, nrows, ncols, PHIin, S_in, None, ctypes.addressof(prm), ctypes.c_ulonglong(0),
                  ctypes.addressof(s_out), PTR + 4096, PTR, PTR)
    assert e.value.code == capi.PDEIP_ERR_ARG, str(e.value)
    assert s_out.value == -7
    return str(e.value)


def test_disp_segmentation_refusals(pdeip):
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
