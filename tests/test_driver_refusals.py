"""CPU: the eight resident whole-driver entry points (include/pdeip.h, csrc/pdeip_drivers.hip) refuse what they refuse BEFORE any HIP
call, with the same code, text and precedence for every driver -- there is no GPU here, so a refusal that came after a HIP call would
report PDEIP_ERR_DEVICE instead.  The data pointers of a refused call are never dereferenced: they are small fake addresses."""
import ctypes

import numpy as np
import pytest

A, B = 64, 128              # distinct non-NULL input addresses that a refused call must not touch
OUT, OUT2 = 1024, 2048
RGB, GRAD, GRADMAG = 1, 2, 3


def _struct(doubles, ints, **kw):
    class P(ctypes.Structure):
        _fields_ = [(k, ctypes.c_double) for k in doubles] + [(k, ctypes.c_int) for k in ints]
    return P(**kw)


def _driver(**kw):   # pdeip_driver_params
    return _struct(("alpha", "omega", "gammaS", "b1", "b2", "scl_factor"), ("firstLoop", "secondLoop", "iter", "solver", "scales"), **kw)


def _fas(**kw):      # pdeip_fas_params
    return _struct(("alpha", "omega", "b1", "b2", "scl_factor"), ("firstLoop", "iter", "solver", "cycle_index", "scales"), **kw)


def _sym(**kw):      # pdeip_sym_params
    return _struct(("alpha", "beta", "omega", "b1", "b2", "scl_factor"), ("firstLoop", "secondLoop", "iter", "solver"), **kw)


def _tv(**kw):       # pdeip_tv_params
    return _struct(("alpha", "omega", "scl", "scl_factor"), ("outer_iter", "inner_iter", "solver"), **kw)


# entry point -> (parameter struct, the pointer arguments in argument order, has term codes, checks scl_factor, argument list)
def _flow_nd(a):
    return (a["Iin"], a["rows"], a["cols"], a["ch"], a["fst"], a["snd"], a["prm"], None, None, a["U"], a["V"])


def _flow_ad(a):
    return (a["Iin"], a["rows"], a["cols"], a["ch"], a["fst"], a["snd"], a["prm"], a.get("quantile", 0.0), 0, None, None, a["U"], a["V"])


def _flow_plain(a):   # pdeip_flow_hs_elin, pdeip_flow_fas_fmg_elin
    return (a["Iin"], a["rows"], a["cols"], a["ch"], a["prm"], a["U"], a["V"])


def _disp_sym(a):
    return (a["Il"], a["Ir"], a["rows"], a["cols"], a["ch"], a["prm"], a["U"])


def _disp_nd(a):
    return (a["Il"], a["Ir"], a["rows"], a["cols"], a["ch"], a["fst"], a["snd"], a["prm"], None, a["U"])


def _tv_args(a):
    return (a["Iin"], a["rows"], a["cols"], a["ch"], a["prm"], a["Iout"])


FLOW_PTRS = (("Iin", A), ("U", OUT), ("V", OUT2))
STEREO_PTRS = (("Il", A), ("Ir", B), ("U", OUT))
TV_PTRS = (("Iin", A), ("Iout", OUT))
ENTRIES = {
    "pdeip_flow_nd_llin": dict(prm=_driver, ptrs=FLOW_PTRS, terms=True, scl=True, args=_flow_nd),
    "pdeip_flow_ad_llin": dict(prm=_driver, ptrs=FLOW_PTRS, terms=True, scl=True, args=_flow_ad),
    "pdeip_flow_hs_elin": dict(prm=_driver, ptrs=FLOW_PTRS, terms=False, scl=True, args=_flow_plain),
    "pdeip_flow_fas_fmg_elin": dict(prm=_fas, ptrs=FLOW_PTRS, terms=False, scl=False, args=_flow_plain),
    "pdeip_disp_nd_llin": dict(prm=_driver, ptrs=STEREO_PTRS, terms=True, scl=True, args=_disp_nd),
    "pdeip_disp_nd_llin_sym": dict(prm=_sym, ptrs=STEREO_PTRS, terms=False, scl=True, args=_disp_sym),
    "pdeip_tvdenoise8": dict(prm=_tv, ptrs=TV_PTRS, terms=False, scl=True, args=_tv_args),
    "pdeip_tvdenoise4": dict(prm=_tv, ptrs=TV_PTRS, terms=False, scl=True, args=_tv_args),
}


def _refused(capi, code, name, prm=None, **kw):
    """The call is refused with `code`, names its entry point, and the text is returned.  prm: keywords of the entry's parameter struct."""
    e = ENTRIES[name]
    p = e["prm"](**prm) if prm else None   # kept alive until the call returns
    a = dict(e["ptrs"], rows=32, cols=40, ch=1, fst=RGB, snd=0, prm=None if p is None else ctypes.addressof(p))
    a.update(kw)
    with pytest.raises(capi.PdeipError) as err:
        capi.call(name, *e["args"](a))
    assert err.value.code == code, "%s: %s" % (name, err.value)
    assert name in str(err.value)
    return str(err.value)


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_refusals_and_their_precedence(pdeip, name):
    capi = pdeip.capi
    ARG, SOLVER = capi.PDEIP_ERR_ARG, capi.PDEIP_ERR_SOLVER
    e = ENTRIES[name]
    ptrs = [k for k, _ in e["ptrs"]]
    for k, ptr in enumerate(ptrs):   # each NULL pointer; of two, the earlier argument is named
        assert "argument '%s' is NULL" % ptr in _refused(capi, ARG, name, **{ptr: None})
        assert "argument '%s' is NULL" % ptr in _refused(capi, ARG, name, **dict.fromkeys(ptrs[k:]))
    assert "at least 3x3 (got 2x8)" in _refused(capi, ARG, name, rows=2, cols=8)
    assert "at least 3x3 (got 8x2)" in _refused(capi, ARG, name, rows=8, cols=2)
    assert "frames must be >= 1 (got 0)" in _refused(capi, ARG, name, ch=0)
    assert "more than 2^31-1 elements" in _refused(capi, ARG, name, rows=46341, cols=46341)
    assert "more than 2^31-1 elements" in _refused(capi, ARG, name, rows=32768, cols=32768, ch=2)
    assert "is NULL" in _refused(capi, ARG, name, rows=2, cols=8, **{ptrs[-1]: None})   # a NULL output and bad dims: the NULL
    if e["terms"]:
        for fst in (0, GRADMAG, 4, -1):
            assert "No such fstTerm" in _refused(capi, ARG, name, fst=fst)
        for snd in (GRAD, 4, -1):
            assert "No such sndTerm" in _refused(capi, ARG, name, snd=snd)
        assert "No such fstTerm" in _refused(capi, ARG, name, fst=7, snd=7)
        assert "at least 3x3" in _refused(capi, ARG, name, rows=2, cols=8, fst=7)            # bad dims and a bad term: the dims
        assert "frames" in _refused(capi, ARG, name, ch=0, snd=9)
        assert "No such sndTerm" in _refused(capi, ARG, name, snd=9, prm=dict(solver=3))    # the terms come before the parameters
    for solver in (3, 7):
        assert "no such solver" in _refused(capi, SOLVER, name, prm=dict(solver=solver))
    assert "no such solver" in _refused(capi, SOLVER, name, prm=dict(solver=3, scl_factor=1.5))   # a bad solver and a bad scl_factor: the solver
    assert "at least 3x3" in _refused(capi, ARG, name, rows=2, cols=8, prm=dict(solver=3))
    if e["scl"]:
        for scl in (1.0, 1.5):
            assert "scl_factor must be below 1" in _refused(capi, ARG, name, prm=dict(scl_factor=scl))


def test_anisotropic_driver_checks_its_quantile_last(pdeip):
    capi = pdeip.capi
    name = "pdeip_flow_ad_llin"
    for q in (1.0000001, 2.0):
        assert "quantile must be in (0, 1]" in _refused(capi, capi.PDEIP_ERR_ARG, name, quantile=q)
    assert "scl_factor must be below 1" in _refused(capi, capi.PDEIP_ERR_ARG, name, quantile=2.0, prm=dict(scl_factor=1.0))
    assert "no such solver" in _refused(capi, capi.PDEIP_ERR_SOLVER, name, quantile=2.0, prm=dict(solver=5))


def test_fas_driver_does_not_check_scl_factor(pdeip):
    """pdeip_flow_fas_fmg_elin halves its pyramid whatever scl_factor says (it only scales the restriction and the prolongation): 1.0
    and 1.5 get past the entry's checks.  Without a GPU the call then ends at the first HIP call, PDEIP_ERR_DEVICE; with one it runs --
    so this call, unlike the refused ones, is given real frames."""
    capi = pdeip.capi
    I = np.asfortranarray(np.linspace(0.0, 255.0, 16 * 20 * 2, dtype=np.float32).reshape(16, 20, 2))
    U, V = np.zeros((16, 20), np.float32, order="F"), np.zeros((16, 20), np.float32, order="F")
    for scl in (1.0, 1.5):
        p = _fas(scl_factor=scl, scales=1, firstLoop=1, iter=1)
        try:
            capi.call("pdeip_flow_fas_fmg_elin", I.ctypes.data, 16, 20, 1, ctypes.addressof(p), U.ctypes.data, V.ctypes.data)
        except capi.PdeipError as err:   # no GPU: past the checks, stopped by the first HIP call
            assert err.code == capi.PDEIP_ERR_DEVICE, str(err)
            assert "scl_factor" not in str(err)
        else:                            # a call that returns means a GPU ran it: past the checks as well, and intended
            assert np.isfinite(U).all() and np.isfinite(V).all()
