"""CPU: the region-competition entry points refuse what include/pdeip.h says they refuse BEFORE any HIP call -- there is no GPU
here, so a refusal that came after one would report PDEIP_ERR_DEVICE instead.  The pointers are never dereferenced."""
import ctypes
import math

import pytest

PTR = 64  # a non-NULL address that a refused call must not touch


def _level(capi, nrows=8, ncols=8, S=2, order=1, strategy=2, minCOV=1.0, cset=0.5, iterations=3, srem=0.01, prm=None):
    s_out = ctypes.c_int(-7)
    with pytest.raises(capi.PdeipError) as e:
        capi.call("pdeip_seg_competition_level_dev", None, PTR, PTR, nrows, ncols, S, order, strategy, minCOV, cset, iterations, srem,
                  ctypes.c_ulonglong(0), None, prm, ctypes.addressof(s_out), PTR + 4096, PTR, PTR, None)
    assert e.value.code == capi.PDEIP_ERR_ARG, str(e.value)
    assert s_out.value == -7
    return str(e.value)


class _Prm(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in ("c0", "c1", "dh_floor", "err_thr", "gamma_coef", "dist_cap", "nan_fill")]


def test_level_refusals(pdeip):
    capi = pdeip.capi
    assert "2x2" in _level(capi, nrows=1)
    assert "2x2" in _level(capi, ncols=1)
    assert "segments" in _level(capi, S=0)
    assert "order" in _level(capi, order=3)
    assert "strategy" in _level(capi, strategy=3)
    assert "strategy" in _level(capi, strategy=-1)
    for bad in (math.nan, math.inf):
        assert "finite" in _level(capi, minCOV=bad)
        assert "finite" in _level(capi, srem=bad)
        assert "finite" in _level(capi, cset=bad)
    inf_thr = _Prm(*([math.nan] * 3 + [math.inf] + [math.nan] * 3))
    assert "finite" in _level(capi, prm=ctypes.addressof(inf_thr))
    assert "minCOV" in _level(capi, minCOV=0.0)
    assert "minCOV" in _level(capi, minCOV=-1.0)
    assert "iterations" in _level(capi, iterations=-1)


def test_host_forms_and_stages_refuse_before_any_hip_call(pdeip):
    capi = pdeip.capi
    calls = (
        ("pdeip_seg_competition_level", (PTR, PTR, 8, 8, 0, 1, 2, 1.0, 0.5, 3, 0.01, ctypes.c_ulonglong(0), None, None, PTR, PTR, PTR, PTR, None)),
        ("pdeip_region_competition", (PTR, PTR, 8, 8, 2, 1, 7, 1.0, 0.5, 3, 0.01, 0.7, 0.4, ctypes.c_ulonglong(0), None, PTR, PTR, PTR, PTR)),
        ("pdeip_region_competition", (PTR, PTR, 8, 8, 2, 1, 2, 1.0, 0.5, 3, 0.01, 1.5, 0.4, ctypes.c_ulonglong(0), None, PTR, PTR, PTR, PTR)),
        ("pdeip_seg_sizes_dev", (None, PTR, 1, 8, 2, PTR)),
        ("pdeip_seg_variance_dev", (None, PTR, PTR, 8, 8, 2, 0.0, math.inf, PTR, None)),
        ("pdeip_seg_data_dev", (None, PTR, PTR, PTR, PTR, 8, 8, 2, 5, PTR + 4096, None)),
        ("pdeip_seg_label_dev", (None, PTR, 8, 8, 0, PTR)),
        ("pdeip_seg_label", (PTR, 8, 1, 2, PTR)),
        ("pdeip_seg_label", (None, 8, 8, 2, PTR)),
    )
    for name, args in calls:
        with pytest.raises(capi.PdeipError) as e:
            capi.call(name, *args)
        assert e.value.code == capi.PDEIP_ERR_ARG, "%s: %s" % (name, e.value)
