"""CPU: the hole-filling entry points (include/pdeip.h, csrc/pdeip_inpaint.hip) refuse what the header says they refuse BEFORE any HIP
call -- there is no GPU here, so a refusal that came after one would report PDEIP_ERR_DEVICE instead.  The data pointers are never
dereferenced.  The Python drivers reject bad parameters before they reach the library."""
import ctypes
import importlib
import math

import numpy as np
import pytest

A, B, C = 64, 128, 192   # distinct non-NULL addresses that a refused call must not touch
OUT = 1024
W = (2048, 2112, 2176, 2240, 2304, 2368)   # TRACE, B and the four weight planes


def _refused(capi, code, name, *args):
    with pytest.raises(capi.PdeipError) as e:
        capi.call(name, *args)
    assert e.value.code == code, str(e.value)
    assert name in str(e.value)
    return str(e.value)


def _prm(pdeip, **kw):
    dev_params = importlib.import_module("pde-based-image-processing_amd.device").InpaintParams
    p = dev_params.make(**kw)
    return p, ctypes.addressof(p)


def test_stage_refusals(pdeip):
    capi = pdeip.capi
    ARG, UNS = capi.PDEIP_ERR_ARG, capi.PDEIP_ERR_UNSUPPORTED
    name = "pdeip_nan_resize_dev"
    assert "'in' is NULL" in _refused(capi, ARG, name, None, None, 8, 8, 1, 4, 4, 0.5, OUT)
    assert "'out' is NULL" in _refused(capi, ARG, name, None, A, 8, 8, 1, 4, 4, 0.5, None)
    assert "at least 3x3" in _refused(capi, ARG, name, None, A, 2, 8, 1, 4, 4, 0.5, OUT)
    assert "at least 3x3" in _refused(capi, ARG, name, None, A, 8, 8, 1, 4, 2, 0.5, OUT)
    assert "frames" in _refused(capi, ARG, name, None, A, 8, 8, 0, 4, 4, 0.5, OUT)
    assert "alias" in _refused(capi, ARG, name, None, A, 8, 8, 1, 4, 4, 0.5, A)
    for cover in (0.0, -0.25, 1.0000001, math.nan, math.inf):
        assert "cover" in _refused(capi, ARG, name, None, A, 8, 8, 1, 4, 4, cover, OUT)
    assert "taps" in _refused(capi, UNS, name, None, A, 80, 80, 1, 8, 40, 0.5, OUT)
    assert "columns" in _refused(capi, UNS, name, None, A, 3, 65536, 1, 3, 65536, 0.5, OUT)

    name = "pdeip_inpaint_meanfill_dev"
    assert "'D' is NULL" in _refused(capi, ARG, name, None, None, 8, 8, 1, OUT)
    assert "'out' is NULL" in _refused(capi, ARG, name, None, A, 8, 8, 1, None)
    assert "at least 3x3" in _refused(capi, ARG, name, None, A, 8, 0, 1, OUT)
    assert "2^31-1" in _refused(capi, ARG, name, None, A, 46341, 46341, 1, OUT)

    name = "pdeip_tv4_inpaint_assemble_dev"
    args = lambda X=A, D=B, g=None, gc=0, rows=8, cols=8, F=1, outs=W: (None, X, D, g, gc, 20.0, rows, cols, F, 5.0) + tuple(outs)
    assert "'X' is NULL" in _refused(capi, ARG, name, *args(X=None))
    assert "'D' is NULL" in _refused(capi, ARG, name, *args(D=None))
    for k, what in enumerate(("TRACE", "B", "wW", "wN", "wE", "wS")):
        outs = list(W)
        outs[k] = None
        assert "'%s' is NULL" % what in _refused(capi, ARG, name, *args(outs=outs))
    assert "at least 3x3" in _refused(capi, ARG, name, *args(rows=2))
    assert "guide_channels must be >= 0" in _refused(capi, ARG, name, *args(g=C, gc=-1))
    assert "guide is given but guide_channels is 0" in _refused(capi, ARG, name, *args(g=C, gc=0))
    assert "guide is NULL but guide_channels is 2" in _refused(capi, ARG, name, *args(g=None, gc=2))

    name = "pdeip_inpaint_merge_dev"
    assert "'X' is NULL" in _refused(capi, ARG, name, None, None, B, 8, 8, 1, OUT, None)
    assert "'D' is NULL" in _refused(capi, ARG, name, None, A, None, 8, 8, 1, OUT, None)
    assert "'out' is NULL" in _refused(capi, ARG, name, None, A, B, 8, 8, 1, None, OUT)
    assert "at least 3x3" in _refused(capi, ARG, name, None, A, B, 8, 1, 1, OUT, None)


def test_driver_refusals(pdeip):
    capi = pdeip.capi
    ARG, UNS = capi.PDEIP_ERR_ARG, capi.PDEIP_ERR_UNSUPPORTED
    for name, lead in (("pdeip_tv_inpaint4_dev", (None,)), ("pdeip_tv_inpaint4", ())):
        call = lambda D=A, rows=32, cols=40, F=1, g=None, gc=0, prm=None, out=OUT: _refused(capi, ARG, name, *lead, D, rows, cols, F, g, gc, prm, out, None)
        assert "'D' is NULL" in call(D=None)
        assert "'out' is NULL" in call(out=None)
        for rows, cols in ((2, 40), (32, 2), (0, 40), (32, -1)):
            assert "at least 3x3" in call(rows=rows, cols=cols)
        assert "frames" in call(F=0)
        assert "2^31-1" in call(rows=46341, cols=46341)
        assert "guide_channels must be >= 0" in call(g=C, gc=-3)
        assert "guide is given but guide_channels is 0" in call(g=C)
        assert "guide is NULL but guide_channels is 1" in call(gc=1)
        for scl in (1.0, 1.5, math.inf):
            p, ptr = _prm(pdeip, scl_factor=scl)
            assert "scl_factor must be below 1" in call(prm=ptr)
        for cover in (1.0000001, 2.0, math.inf):
            p, ptr = _prm(pdeip, cover=cover)
            assert "cover must not be above 1" in call(prm=ptr)
        for solver in (3, 7):
            p, ptr = _prm(pdeip, solver=solver)
            assert "unknown solver %d" % solver in call(prm=ptr)
        p, ptr = _prm(pdeip, alpha=1e39)
        assert "finite in single" in call(prm=ptr)
        p, ptr = _prm(pdeip, scl_factor=0.05, min_size=3)
        assert "taps" in _refused(capi, UNS, name, *lead, A, 200, 200, 1, None, 0, ptr, OUT, None)
        assert "columns" in _refused(capi, UNS, name, *lead, A, 3, 65536, 1, None, 0, None, OUT, None)


def test_python_drivers_refuse_before_the_library(pdeip):
    drv = importlib.import_module("pde-based-image-processing_amd.drivers")
    D = np.zeros((20, 24), np.float32)
    for fn in (drv.TVinpaint4, drv.capi_TVinpaint4):
        with pytest.raises(ValueError, match=r"\[rows, cols\]"):
            fn(np.zeros(5, np.float32))
        with pytest.raises(ValueError, match="guide"):
            fn(D, guide=np.zeros((20, 25), np.float32))
    with pytest.raises(ValueError, match="scl_factor"):
        drv.TVinpaint4(D, scl_factor=1.0)
    with pytest.raises(ValueError, match="cover"):
        drv.TVinpaint4(D, cover=1.5)
    with pytest.raises(ValueError, match="solver"):
        drv.TVinpaint4(D, solver=4)
    with pytest.raises(ValueError, match="unknown parameter"):
        drv.TVinpaint4(D, alhpa=3.0)
    with pytest.raises(ValueError, match="scl_factor"):
        drv.stereo_maps(D, D, fill=True, fill_param=dict(scl_factor=2.0))
