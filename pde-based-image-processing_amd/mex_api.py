"""Host-side mirror of the reference's MEX gateways (mex/source/*.c) over libpdeip.so.

Each function has the gateway's name, argument order and meaning; arrays are numpy float32
with MATLAB's shape convention ([nrows, ncols] or [nrows, ncols, nframes]) and are handed to
the C-ABI in column-major (Fortran) order, which is exactly the memory a MATLAB `single` array
has.  `nargout` plays the role of MATLAB's nlhs.  Errors the gateways raise through
mexErrMsgTxt (wrong type, too few outputs, unknown solver) surface as MexError with the same
kind of message.

All arithmetic happens in libpdeip.so on the GPU; this file only checks, packs and unpacks.

Reference: Oflow_sor_elin4_2d.c, Oflow_sor_llin4_2d.c, Oflow_sor_llin8_2d.c, Oflow_lhs_elin4_2d.c,
Oflow_lhs_llin4_2d.c, Disp_sor_llin4_2d.c, PDEsolver4.c, PDEsolver8.c, DdiffWeights.c,
BilinInterp_2d.c, FstDerivatives5.c, SndDerivatives5.c, AC_solver_2d.c, Reinit.c, CV_solver_2d.c, SurfaceEquation.c (all under
mex/source/).
"""
import numpy as np

from . import capi


class MexError(capi.PdeipError):
    """What MATLAB would report after mexErrMsgTxt."""


def _single(name, who, a):
    """mxIsSingle check of the gateways (e.g. Oflow_sor_elin4_2d.c:117-119)."""
    if not isinstance(a, np.ndarray) or a.dtype != np.float32:
        raise MexError(capi.PDEIP_ERR_ARG, "%s: '%s' must be a noncomplex single-valued matrix." % (who, name))
    if a.ndim == 1:
        a = a.reshape(-1, 1)
    if a.ndim not in (2, 3):
        raise MexError(capi.PDEIP_ERR_ARG, "%s: '%s' must have 2 or 3 dimensions." % (who, name))
    return np.asfortranarray(a)


def _scalar(name, who, v):
    """Scalars cross the MEX boundary as 1x1 singles (Oflow_sor_elin4_2d.c:260-283)."""
    a = np.asarray(v)
    if a.dtype != np.float32 or a.size != 1:
        raise MexError(capi.PDEIP_ERR_ARG, "%s: '%s' must be a noncomplex, single-type scalar" % (who, name))
    return float(a.reshape(()))


def _same_plane(who, ref, **arrays):
    for name, a in arrays.items():
        if a.shape[:2] != ref.shape[:2]:
            raise MexError(capi.PDEIP_ERR_ARG, "%s: '%s' is %s but the image is %s" %
                           (who, name, a.shape[:2], ref.shape[:2]))


def _ptr(a):
    return a.ctypes.data if a is not None else None


def _frames(a):
    return a.shape[2] if a.ndim == 3 else 1


def _run(fn, *args):
    try:
        capi.call(fn, *args)
    except capi.PdeipError as exc:
        raise MexError(exc.code, str(exc)) from None


def _out_like(a):
    return np.zeros(a.shape, dtype=np.float32, order="F")  # mxCreateNumericArray zero-fills


def _oflow_sor(who, fn, planes, weights, it, omega, solver, nargout, iterate_names):
    if nargout < 2:
        raise MexError(capi.PDEIP_ERR_ARG, "%s insufficient number of outputs." % who)
    arrs = [_single(n, who, a) for n, a in planes]
    wts = [_single(n, who, a) for n, a in weights]
    it = _scalar("iter", who, it)
    omega = _scalar("omega", who, omega)
    solver = int(_scalar("solver", who, solver))
    named = dict(zip([n for n, _ in planes], arrs))
    ref = named[iterate_names[0]]
    _same_plane(who, ref, **dict(zip([n for n, _ in planes + weights], arrs + wts)))
    M = named["M"]
    F = _frames(M)
    for n in ("Cu", "Cv", "Du", "Dv"):
        if _frames(named[n]) != F:
            raise MexError(capi.PDEIP_ERR_ARG, "%s: '%s' must have as many frames as 'M'" % (who, n))
    o0, o1 = _out_like(named[iterate_names[0]]), _out_like(named[iterate_names[1]])
    RU = RV = None
    if nargout >= 4:  # residual outputs take M's dimensions (Oflow_sor_elin4_2d.c:309-325)
        RU, RV = _out_like(M), _out_like(M)
    nrows, ncols = ref.shape[:2]
    _run(fn, *[_ptr(a) for a in arrs + wts], nrows, ncols, F, int(it), omega, solver,
         _ptr(o0), _ptr(o1), _ptr(RU), _ptr(RV))
    return (o0, o1) if nargout < 4 else (o0, o1, RU, RV)


def Oflow_sor_elin4_2d(U, V, M, Cu, Cv, Du, Dv, wW, wN, wE, wS, iter, omega, solver, nargout=2):
    """[U,V(,RU,RV)] = Oflow_sor_elin4_2d(...)  -- mex/source/Oflow_sor_elin4_2d.c:64-352."""
    return _oflow_sor("Oflow_sor_elin4_2d", "pdeip_oflow_sor_elin4",
                      [("U", U), ("V", V), ("M", M), ("Cu", Cu), ("Cv", Cv), ("Du", Du), ("Dv", Dv)],
                      [("wW", wW), ("wN", wN), ("wE", wE), ("wS", wS)], iter, omega, solver, nargout, ("U", "V"))


def Oflow_sor_llin4_2d(U, V, dU, dV, M, Cu, Cv, Du, Dv, wW, wN, wE, wS, iter, omega, solver, nargout=2):
    """[dU,dV(,RU,RV)] = Oflow_sor_llin4_2d(...)  -- mex/source/Oflow_sor_llin4_2d.c:66-386."""
    return _oflow_sor("Oflow_sor_llin4_2d", "pdeip_oflow_sor_llin4",
                      [("U", U), ("V", V), ("dU", dU), ("dV", dV), ("M", M), ("Cu", Cu), ("Cv", Cv), ("Du", Du),
                       ("Dv", Dv)],
                      [("wW", wW), ("wN", wN), ("wE", wE), ("wS", wS)], iter, omega, solver, nargout, ("dU", "dV"))


def Oflow_sor_llin8_2d(U, V, dU, dV, M, Cu, Cv, Du, Dv, wW, wNW, wN, wNE, wE, wSE, wS, wSW, iter, omega, solver,
                       nargout=2):
    """[dU,dV(,RU,RV)] = Oflow_sor_llin8_2d(...)  -- mex/source/Oflow_sor_llin8_2d.c:71-489."""
    return _oflow_sor("Oflow_sor_llin8_2d", "pdeip_oflow_sor_llin8",
                      [("U", U), ("V", V), ("dU", dU), ("dV", dV), ("M", M), ("Cu", Cu), ("Cv", Cv), ("Du", Du),
                       ("Dv", Dv)],
                      [("wW", wW), ("wNW", wNW), ("wN", wN), ("wNE", wNE), ("wE", wE), ("wSE", wSE), ("wS", wS),
                       ("wSW", wSW)], iter, omega, solver, nargout, ("dU", "dV"))


def _oflow_lhs(who, fn, planes, weights, nargout):
    if nargout < 2:
        raise MexError(capi.PDEIP_ERR_ARG, "%s insufficient number of outputs." % who)
    arrs = [_single(n, who, a) for n, a in planes]
    wts = [_single(n, who, a) for n, a in weights]
    named = dict(zip([n for n, _ in planes], arrs))
    ref = named["U"]
    _same_plane(who, ref, **dict(zip([n for n, _ in planes + weights], arrs + wts)))
    M = named["M"]
    F = _frames(M)
    AU, AV = _out_like(M), _out_like(M)  # outputs take M's dimensions (Oflow_lhs_elin4_2d.c:207-227)
    nrows, ncols = ref.shape[:2]
    _run(fn, *[_ptr(a) for a in arrs + wts], nrows, ncols, F, _ptr(AU), _ptr(AV))
    return AU, AV


def Oflow_lhs_elin4_2d(U, V, M, Du, Dv, wW, wN, wE, wS, nargout=2):
    """[AU,AV] = Oflow_lhs_elin4_2d(...)  -- mex/source/Oflow_lhs_elin4_2d.c:56-231."""
    return _oflow_lhs("Oflow_lhs_elin4_2d", "pdeip_oflow_lhs_elin4",
                      [("U", U), ("V", V), ("M", M), ("Du", Du), ("Dv", Dv)],
                      [("wW", wW), ("wN", wN), ("wE", wE), ("wS", wS)], nargout)


def Oflow_lhs_llin4_2d(U, V, dU, dV, M, Du, Dv, wW, wN, wE, wS, nargout=2):
    """[AU,AV] = Oflow_lhs_llin4_2d(...)  -- mex/source/Oflow_lhs_llin4_2d.c:59-260."""
    return _oflow_lhs("Oflow_lhs_llin4_2d", "pdeip_oflow_lhs_llin4",
                      [("U", U), ("V", V), ("dU", dU), ("dV", dV), ("M", M), ("Du", Du), ("Dv", Dv)],
                      [("wW", wW), ("wN", wN), ("wE", wE), ("wS", wS)], nargout)


def Disp_sor_llin4_2d(U, dU, Cu, Du, wW, wN, wE, wS, iter, omega, solver, nargout=1):
    """[dU(,RU)] = Disp_sor_llin4_2d(...)  -- mex/source/Disp_sor_llin4_2d.c:59-282."""
    who = "Disp_sor_llin4_2d"
    if nargout < 1:
        raise MexError(capi.PDEIP_ERR_ARG, "%s insufficient number of outputs." % who)
    names = ["U", "dU", "Cu", "Du", "wW", "wN", "wE", "wS"]
    arrs = [_single(n, who, a) for n, a in zip(names, [U, dU, Cu, Du, wW, wN, wE, wS])]
    it, omega, solver = _scalar("iter", who, iter), _scalar("omega", who, omega), int(_scalar("solver", who, solver))
    _same_plane(who, arrs[0], **dict(zip(names, arrs)))
    out = _out_like(arrs[1])
    RU = _out_like(arrs[0]) if nargout >= 2 else None
    nrows, ncols = arrs[0].shape[:2]
    _run("pdeip_disp_sor_llin4", *[_ptr(a) for a in arrs], nrows, ncols, int(it), omega, solver, _ptr(out), _ptr(RU))
    return out if nargout < 2 else (out, RU)


def Disp_sor_llin_sym4_2d(U0, dU0, Cu0, Du0, wW0, wN0, wE0, wS0, U1, dU1, Cu1, Du1, wW1, wN1, wE1, wS1, iter, omega, solver,
                          nargout=2):
    """[dU0 dU1] = Disp_sor_llin_sym4_2d(...)  -- mex/source/Disp_sor_llin_sym4_2d.c:82-440."""
    who = "Disp_sor_llin_sym4_2d"
    if nargout < 2:
        raise MexError(capi.PDEIP_ERR_ARG, "%s insufficient number of outputs." % who)
    names = ["U_in0", "dU_in0", "Cu0", "Du0", "wW0", "wN0", "wE0", "wS0", "U_in1", "dU_in1", "Cu1", "Du1", "wW1", "wN1", "wE1", "wS1"]
    arrs = [_single(n, who, a) for n, a in zip(names, [U0, dU0, Cu0, Du0, wW0, wN0, wE0, wS0, U1, dU1, Cu1, Du1, wW1, wN1, wE1, wS1])]
    it, omega, solver = _scalar("iter", who, iter), _scalar("omega", who, omega), int(_scalar("solver", who, solver))
    _same_plane(who, arrs[0], **dict(zip(names, arrs)))
    o0, o1 = _out_like(arrs[1]), _out_like(arrs[9])
    nrows, ncols = arrs[0].shape[:2]
    _run("pdeip_disp_sor_llin_sym4", *[_ptr(a) for a in arrs], nrows, ncols, int(it), omega, solver, _ptr(o0), _ptr(o1))
    return o0, o1


def _pde(who, fn, names, arrays, it, omega, solver, nargout):
    if nargout < 1:
        raise MexError(capi.PDEIP_ERR_ARG, "%s: error insufficient number of outputs." % who)
    arrs = [_single(n, who, a) for n, a in zip(names, arrays)]
    it, omega, solver = _scalar("iter", who, it), _scalar("omega", who, omega), int(_scalar("solver", who, solver))
    X = arrs[0]
    for n, a in zip(names, arrs):
        if a.shape != X.shape:
            raise MexError(capi.PDEIP_ERR_ARG, "%s: '%s' is %s but X is %s" % (who, n, a.shape, X.shape))
    out = _out_like(X)
    nrows, ncols = X.shape[:2]
    _run(fn, *[_ptr(a) for a in arrs], nrows, ncols, _frames(X), int(it), omega, solver, _ptr(out))
    return out


def PDEsolver4(X, TRACE, B, wW, wN, wE, wS, iter, omega, solver, nargout=1):
    """X = PDEsolver4(...)  -- mex/source/PDEsolver4.c:54-249."""
    return _pde("PDEsolver4", "pdeip_pde_sor4", ["X", "TRACE", "B", "wW", "wN", "wE", "wS"],
                [X, TRACE, B, wW, wN, wE, wS], iter, omega, solver, nargout)


def PDEsolver8(X, TRACE, B, wW, wNW, wN, wNE, wE, wSE, wS, wSW, iter, omega, solver, nargout=1):
    """X = PDEsolver8(...)  -- mex/source/PDEsolver8.c:54-309."""
    return _pde("PDEsolver8", "pdeip_pde_sor8",
                ["X", "TRACE", "B", "wW", "wNW", "wN", "wNE", "wE", "wSE", "wS", "wSW"],
                [X, TRACE, B, wW, wNW, wN, wNE, wE, wSE, wS, wSW], iter, omega, solver, nargout)


def DdiffWeights(D, eps, nargout=4):
    """[wW,wN,wE,wS] = DdiffWeights(D,eps)  -- mex/source/DdiffWeights.c:50-140."""
    who = "DdiffWeights"
    if nargout < 4:
        raise MexError(capi.PDEIP_ERR_ARG, "diffusion6_2d error insufficient number of outputs. Outputs from this "
                                            "function are 'wW', 'wN', 'wE' and 'wS'")
    D = _single("D", who, D)
    eps = _scalar("eps", who, eps)
    outs = [_out_like(D) for _ in range(4)]
    nrows, ncols = D.shape[:2]
    _run("pdeip_diffweights6", _ptr(D), nrows, ncols, _frames(D), eps, *[_ptr(o) for o in outs])
    return tuple(outs)


def BilinInterp_2d(Iin, X, Y, nargout=1):
    """Iout = BilinInterp_2d(Iin,X,Y)  -- mex/source/BilinInterp_2d.c:41-124."""
    who = "BilinInterp_2d"
    if nargout < 1:
        raise MexError(capi.PDEIP_ERR_ARG, "insufficient number of outputs. Outputs from this function is 'Iout'")
    Iin, X, Y = _single("Iin", who, Iin), _single("X", who, X), _single("Y", who, Y)
    _same_plane(who, Iin, X=X, Y=Y)
    out = _out_like(Iin)
    nrows, ncols = Iin.shape[:2]
    _run("pdeip_warp_bilinear", _ptr(Iin), _ptr(X), _ptr(Y), nrows, ncols, _frames(Iin), _ptr(out))
    return out


def _derivatives(who, fn, It0, It1, nout, nargout, msg):
    if nargout < nout:
        raise MexError(capi.PDEIP_ERR_ARG, msg)
    It0, It1 = _single("It0", who, It0), _single("It1", who, It1)
    if It0.shape != It1.shape:
        raise MexError(capi.PDEIP_ERR_ARG, "%s: 'It1' is %s but 'It0' is %s" % (who, It1.shape, It0.shape))
    outs = [_out_like(It0) for _ in range(nout)]
    nrows, ncols = It0.shape[:2]
    _run(fn, _ptr(It0), _ptr(It1), nrows, ncols, _frames(It0), *[_ptr(o) for o in outs])
    return tuple(outs)


def FstDerivatives5(It0, It1, nargout=3):
    """[Idt,Idx,Idy] = FstDerivatives5(It0,It1)  -- mex/source/FstDerivatives5.c:50-145."""
    return _derivatives("fstDerivatives", "pdeip_fst_derivatives5", It0, It1, 3, nargout,
                        "fstDerivatives: insufficient number of outputs...outputs from this function are 'Idt', 'Idx' and 'Idy'.")


def SndDerivatives5(It0, It1, nargout=5):
    """[Idxt,Idyt,Idxx,Idyy,Idxy] = SndDerivatives5(It0,It1)  -- mex/source/SndDerivatives5.c:51-174."""
    return _derivatives("sndDerivatives", "pdeip_snd_derivatives5", It0, It1, 5, nargout,
                        "sndDerivatives: insufficient number of outputs.")


def AC_solver_2d(PHI, D, GradNorm, Diff, tau, nu, nargout=1):
    """PHI_out = AC_solver_2d(PHI_in,D_in,GradNorm_in,Diff_in,tau,nu)  -- mex/source/AC_solver_2d.c:47-228."""
    who = "AC_solver_2D error"
    planes = [_single(n, who, a) for n, a in (("PHI_in", PHI), ("D_in", D), ("GradNorm_in", GradNorm), ("Diff_in", Diff))]
    tau, nu = _scalar("tau", who, tau), _scalar("nu", who, nu)
    if nargout < 1:
        raise MexError(capi.PDEIP_ERR_ARG, "ac_solver_2D error insufficient number of outputs. Outputs from this function is 'PHI_out'")
    PHI = planes[0]
    if any(a.size != PHI.size for a in planes[1:]):  # the rule and message of mex/levelset/AC_solver_2d.c
        raise MexError(capi.PDEIP_ERR_ARG, "AC_solver_2D error: 'D_in', 'GradNorm_in' and 'Diff_in' must have the size of 'PHI_in'.")
    out = _out_like(PHI)
    nrows, ncols = PHI.shape[:2]
    _run("pdeip_ac_solver", *[_ptr(a) for a in planes], nrows, ncols, _frames(PHI), tau, nu, _ptr(out))
    return out


def CV_solver_2d(PHI, D, DH, GradNorm, tau, nu, nargout=1):
    """PHI_out = CV_solver_2d(PHI_in,D_in,DH_in,GradNorm_in,tau,nu)  -- mex/source/CV_solver_2d.c (-> CV_AOSOMP_4_2d)."""
    who = "cv_solver_2D error"
    planes = [_single(n, who, a) for n, a in (("PHI_in", PHI), ("D_in", D), ("DH_in", DH), ("GradNorm_in", GradNorm))]
    tau, nu = _scalar("tau", who, tau), _scalar("nu", who, nu)
    PHI = planes[0]
    if any(a.size != PHI.size for a in planes[1:]):  # the rule and message of mex/levelset/CV_solver_2d.c
        raise MexError(capi.PDEIP_ERR_ARG, "cv_solver_2D error: 'D_in', 'DH_in' and 'GradNorm_in' must have the size of 'PHI_in'.")
    if nargout < 1:
        raise MexError(capi.PDEIP_ERR_ARG, "cv_solver_2D error insufficient number of outputs. Outputs from this function is 'PHI_out'")
    out = _out_like(PHI)
    nrows, ncols = PHI.shape[:2]
    _run("pdeip_cv_solver", *[_ptr(a) for a in planes], nrows, ncols, _frames(PHI), tau, nu, _ptr(out))
    return out


def Reinit(PHI, T, nargout=1):
    """PHI_out = Reinit(PHI_in,T)  -- mex/source/Reinit.c:47-139.  Unlike the reference gateway, PHI_in is left unchanged."""
    PHI = _single("PHI_in", "reInitC", PHI)
    T = _scalar("T", "reInitC error", T)
    if nargout < 1:
        raise MexError(capi.PDEIP_ERR_ARG, "reInitC error insufficient number of outputs. Outputs from this function is 'PHI_out'")
    out = _out_like(PHI)
    nrows, ncols = PHI.shape[:2]
    _run("pdeip_reinit", _ptr(PHI), nrows, ncols, _frames(PHI), T, _ptr(out))
    return out


_surface_seed = None  # the stub's rule: drawn from the clock on the first unseeded call, advanced per call


def surface_equation(A, B, M_in, err_thr, min_set_size, iter, seed=None, sets=None):
    """pdeip_surface_equation on numpy arrays: (M_out [ncoef], Err [ndata], inliers [iter+1], errsum [iter+1]).  A single
    [ndata, ncoef] (column-major), B [ndata], M_in [ncoef] or None, sets uint32 [iter, ncoef+1] or None (then drawn from seed)."""
    global _surface_seed
    import ctypes
    import time

    A = np.asfortranarray(A, dtype=np.float32)
    B = np.ascontiguousarray(B, dtype=np.float32).reshape(-1)
    ndata, ncoef = A.shape
    it = max(int(iter), 0)
    M_in = None if M_in is None else np.ascontiguousarray(M_in, dtype=np.float32).reshape(-1)
    if sets is not None:
        sets = np.ascontiguousarray(sets, dtype=np.uint32)
        if sets.size != it * (ncoef + 1):
            raise MexError(capi.PDEIP_ERR_ARG, "SurfaceEquation: 'sets' must hold iter x (ncoef + 1) indices")
    elif seed is None:
        if _surface_seed is None:
            _surface_seed = int(time.time())
        seed, _surface_seed = _surface_seed, (_surface_seed + 0x9E3779B97F4A7C15) & ((1 << 64) - 1)
    M = np.zeros(ncoef, np.float32)
    err = np.zeros(ndata, np.float32)
    inl = np.zeros(it + 1, np.int32)
    esum = np.zeros(it + 1, np.float64)
    _run("pdeip_surface_equation", _ptr(A), _ptr(B), ndata, ncoef, _ptr(M_in), float(err_thr), float(min_set_size), int(iter), _ptr(sets),
         ctypes.c_ulonglong(int(seed or 0) & ((1 << 64) - 1)), _ptr(M), _ptr(err), _ptr(inl), _ptr(esum))
    return M, err, inl, esum


def SurfaceEquation(A_in, B_in, M_in, err_thr, min_set_size, iter, seed=None, sets=None, nargout=2):
    """[M_out, Err] = SurfaceEquation(A_in,B_in,M_in,err_thr,min_set_size,iter)  -- mex/source/SurfaceEquation.c:69-220.  An empty
    M_in means none; seed / sets: the samples (pdeip.h), without either a seed drawn from the clock once and advanced per call."""
    who = "SurfaceEquation error"
    A = _single("A_in", who, A_in)
    B = _single("B_in", who, B_in)
    M = _single("M_in", who, M_in)
    err_thr, min_set_size = _scalar("err_thr", who, err_thr), _scalar("min_set_size", who, min_set_size)
    iter = _scalar("iter", who, iter)
    if A.ndim != 2 or B.ndim != 2:
        raise MexError(capi.PDEIP_ERR_ARG, "SurfaceEquation error: 'A_in' and 'B_in' must be matrices.")
    if M.size and A.shape[1] != M.shape[0]:
        raise MexError(capi.PDEIP_ERR_ARG, "SurfaceEquation error: M_in is a column vector with as many row elements as A_in has columns!")
    if A.shape[0] != B.shape[0]:
        raise MexError(capi.PDEIP_ERR_ARG, "SurfaceEquation error: A_in and B_in have to have same amount of rows!")
    if A.shape[1] not in (3, 6):
        raise MexError(capi.PDEIP_ERR_ARG, "SurfaceEquation error: only 1st and 2nd order polynomials are implemented!")
    if nargout < 2:
        raise MexError(capi.PDEIP_ERR_ARG, "SurfaceEquation error: insufficient number of outputs. Outputs from this function is 'M_out' and 'error_out'")
    it = int(iter) if iter > 0 else 0  # (unsigned int)iter of the gateway, without its wrap-around for a negative iter
    Mo, err, _, _ = surface_equation(A, B[:, 0], M[:, 0] if M.size else None, err_thr, min_set_size, it, seed, sets)
    return np.asfortranarray(Mo.reshape(-1, 1)), np.asfortranarray(err.reshape(-1, 1))


def set_mode(mode):
    """PDEIP_MODE_EXACT_ORDER (0, default: the reference's sweep order), PDEIP_MODE_RED_BLACK (1) or PDEIP_MODE_LINE_SCAN (2:
    solver = 2 in the reference's line order with each line's recurrences as parallel scans, within 1e-4 RMS of mode 0 on
    diagonally dominant data; every other solver exactly as mode 0)."""
    capi.set_mode(mode)
