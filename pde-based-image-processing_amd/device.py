"""Device-resident calls: the `_dev` entry points of libpdeip.so on torch tensors.

torch is plumbing here (device memory, streams); all arithmetic is in the HIP library.

Layout.  A MATLAB `single` array [nrows x ncols (x F)] in column-major order is, byte for byte, a
C-contiguous array [(F x) ncols x nrows].  Device planes are therefore torch float32 tensors of
shape [ncols, nrows] or [F, ncols, nrows]; `to_device` / `to_matlab` convert from/to the numpy
arrays `mex_api` uses.  Kernels run on torch's current stream.
"""
import ctypes

import numpy as np
import torch

from . import capi


def to_device(a, device="cuda"):
    """numpy [nrows, ncols(, F)] (any order) -> torch [(F,) ncols, nrows] on `device`, same bytes as MATLAB."""
    a = np.asarray(a, dtype=np.float32)
    t = a.transpose(2, 1, 0) if a.ndim == 3 else a.T
    if t.flags.c_contiguous:   # column-major input (what MATLAB holds): its bytes are the device layout already
        return torch.from_numpy(t).to(device)
    # row-major numpy input: upload the bytes as they are and change the layout on the device (a strided host copy of a
    # 1080p colour pair takes longer than the whole resident run)
    d = torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return (d.permute(2, 1, 0) if a.ndim == 3 else d.T).contiguous()


def div_scalar(t, s):
    """t ./ s in float32 with a true division (a Python-scalar divisor would be turned into a multiplication by 1/s)."""
    return t / torch.tensor(s, dtype=torch.float32, device=t.device)


def to_matlab(t):
    """torch [(F,) ncols, nrows] -> numpy [nrows, ncols(, F)] column-major."""
    a = t.detach().cpu().numpy()
    return np.asfortranarray(a.transpose(2, 1, 0) if a.ndim == 3 else a.T)


def _chk(*tensors):
    for t in tensors:
        if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
            raise capi.PdeipError(capi.PDEIP_ERR_ARG, "device planes must be contiguous float32 CUDA tensors")


def _dims(t):
    return int(t.shape[-1]), int(t.shape[-2]), (int(t.shape[0]) if t.dim() == 3 else 1)  # nrows, ncols, F


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """Raw handle of torch's current stream on the current device (the library only enqueues there).  The private accessor
    skips building a Stream object per call -- a solver call on a coarse pyramid scale is shorter than that took."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _p(*ts):
    return [t.data_ptr() for t in ts]


def sync_check():
    """Wait for the device and raise if a bounded dependency wait of the persistent exact-order kernel timed out since
    the last check (the abort word is sticky: later calls cannot clear it).  The resident drivers call this wherever
    they hand results back to the host."""
    torch.cuda.synchronize()
    capi.call("pdeip_persist_error")


def oflow_sor_elin4(U, V, M, Cu, Cv, Du, Dv, wW, wN, wE, wS, iter, omega, mode=capi.MODE_EXACT_ORDER, col0=0, out=None):
    """In place on U, V (GS_SOR_elin4_2d, opticalflowSolvers.c:41); with out=(U2, V2): U, V are only read and the relaxed
    iterate goes to U2, V2 (no device-to-device copy in the red-black mode; callers alternate between two sets)."""
    _chk(U, V, M, Cu, Cv, Du, Dv, wW, wN, wE, wS)
    nrows, ncols, _ = _dims(U)
    if out is None:
        capi.call("pdeip_oflow_sor_elin4_dev", _stream(), *_p(U, V, M, Cu, Cv, Du, Dv, wW, wN, wE, wS), nrows, ncols,
                  int(iter), float(omega), int(mode), int(col0))
    else:
        _chk(*out)
        capi.call("pdeip_oflow_sor_elin4_dev_to", _stream(), *_p(U, V, out[0], out[1], M, Cu, Cv, Du, Dv, wW, wN, wE, wS), nrows,
                  ncols, int(iter), float(omega), int(mode), int(col0))


def oflow_sor_llin4(U, V, dU, dV, M, Cu, Cv, Du, Dv, wW, wN, wE, wS, iter, omega, mode=capi.MODE_EXACT_ORDER, col0=0):
    """In place on dU, dV (GS_SOR_llin4_2d, opticalflowSolvers.c:504)."""
    _chk(U, V, dU, dV, M, Cu, Cv, Du, Dv, wW, wN, wE, wS)
    nrows, ncols, _ = _dims(U)
    capi.call("pdeip_oflow_sor_llin4_dev", _stream(), *_p(U, V, dU, dV, M, Cu, Cv, Du, Dv, wW, wN, wE, wS), nrows,
              ncols, int(iter), float(omega), int(mode), int(col0))


def disp_sor_llin4(U, dU, Cu, Du, wW, wN, wE, wS, iter, omega, mode=capi.MODE_EXACT_ORDER, col0=0):
    """In place on dU (disparitySolvers.c:41)."""
    _chk(U, dU, Cu, Du, wW, wN, wE, wS)
    nrows, ncols, _ = _dims(U)
    capi.call("pdeip_disp_sor_llin4_dev", _stream(), *_p(U, dU, Cu, Du, wW, wN, wE, wS), nrows, ncols, int(iter),
              float(omega), int(mode), int(col0))


def pde_sor4(X, TRACE, B, wW, wN, wE, wS, iter, omega, mode=capi.MODE_EXACT_ORDER, col0=0):
    """In place on X (GS_SOR_4_2d, pdeSolvers.c:44)."""
    _chk(X, TRACE, B, wW, wN, wE, wS)
    nrows, ncols, F = _dims(X)
    capi.call("pdeip_pde_sor4_dev", _stream(), *_p(X, TRACE, B, wW, wN, wE, wS), nrows, ncols, F, int(iter),
              float(omega), int(mode), int(col0))


def pde_sor8(X, TRACE, B, wW, wNW, wN, wNE, wE, wSE, wS, wSW, iter, omega, mode=capi.MODE_EXACT_ORDER, col0=0):
    """In place on X (GS_SOR_8_2d, pdeSolvers.c:153)."""
    _chk(X, TRACE, B, wW, wNW, wN, wNE, wE, wSE, wS, wSW)
    nrows, ncols, F = _dims(X)
    capi.call("pdeip_pde_sor8_dev", _stream(), *_p(X, TRACE, B, wW, wNW, wN, wNE, wE, wSE, wS, wSW), nrows, ncols, F,
              int(iter), float(omega), int(mode), int(col0))


# ---- alternating line relaxation (solver 2); mode EXACT_ORDER = reference line order, RED_BLACK = zebra ----

def oflow_alr_elin4(U, V, M, Cu, Cv, Du, Dv, wW, wN, wE, wS, iter, omega, mode=capi.MODE_EXACT_ORDER):
    """In place on U, V (GS_ALR_SOR_elin4_2d, opticalflowSolvers.c:196)."""
    _chk(U, V, M, Cu, Cv, Du, Dv, wW, wN, wE, wS)
    nrows, ncols, _ = _dims(U)
    capi.call("pdeip_oflow_alr_elin4_dev", _stream(), *_p(U, V, M, Cu, Cv, Du, Dv, wW, wN, wE, wS), nrows, ncols,
              int(iter), float(omega), int(mode))


def oflow_alr_llin4(U, V, dU, dV, M, Cu, Cv, Du, Dv, wW, wN, wE, wS, iter, omega, mode=capi.MODE_EXACT_ORDER):
    """In place on dU, dV (GS_ALR_SOR_llin4_2d, opticalflowSolvers.c:690)."""
    _chk(U, V, dU, dV, M, Cu, Cv, Du, Dv, wW, wN, wE, wS)
    nrows, ncols, _ = _dims(U)
    capi.call("pdeip_oflow_alr_llin4_dev", _stream(), *_p(U, V, dU, dV, M, Cu, Cv, Du, Dv, wW, wN, wE, wS), nrows,
              ncols, int(iter), float(omega), int(mode))


def oflow_alr_llin8(U, V, dU, dV, M, Cu, Cv, Du, Dv, wW, wNW, wN, wNE, wE, wSE, wS, wSW, iter, omega,
                    mode=capi.MODE_EXACT_ORDER):
    """In place on dU, dV (GS_ALR_SOR_llin8_2d, opticalflowSolvers.c:1677)."""
    _chk(U, V, dU, dV, M, Cu, Cv, Du, Dv, wW, wNW, wN, wNE, wE, wSE, wS, wSW)
    nrows, ncols, _ = _dims(U)
    capi.call("pdeip_oflow_alr_llin8_dev", _stream(), *_p(U, V, dU, dV, M, Cu, Cv, Du, Dv, wW, wNW, wN, wNE, wE, wSE, wS, wSW),
              nrows, ncols, int(iter), float(omega), int(mode))


def disp_alr_llin4(U, dU, Cu, Du, wW, wN, wE, wS, iter, omega, mode=capi.MODE_EXACT_ORDER):
    """In place on dU (disparitySolvers.c:154)."""
    _chk(U, dU, Cu, Du, wW, wN, wE, wS)
    nrows, ncols, _ = _dims(U)
    capi.call("pdeip_disp_alr_llin4_dev", _stream(), *_p(U, dU, Cu, Du, wW, wN, wE, wS), nrows, ncols, int(iter),
              float(omega), int(mode))


def pde_alr4(X, TRACE, B, wW, wN, wE, wS, iter, omega, mode=capi.MODE_EXACT_ORDER):
    """In place on X (GS_ALR_SOR_4_2d, pdeSolvers.c:277)."""
    _chk(X, TRACE, B, wW, wN, wE, wS)
    nrows, ncols, F = _dims(X)
    capi.call("pdeip_pde_alr4_dev", _stream(), *_p(X, TRACE, B, wW, wN, wE, wS), nrows, ncols, F, int(iter),
              float(omega), int(mode))


def pde_alr8(X, TRACE, B, wW, wNW, wN, wNE, wE, wSE, wS, wSW, iter, omega, mode=capi.MODE_EXACT_ORDER):
    """In place on X; one iteration whatever `iter` is (GS_ALR_SOR_8_2d, pdeSolvers.c:344)."""
    _chk(X, TRACE, B, wW, wNW, wN, wNE, wE, wSE, wS, wSW)
    nrows, ncols, F = _dims(X)
    capi.call("pdeip_pde_alr8_dev", _stream(), *_p(X, TRACE, B, wW, wNW, wN, wNE, wE, wSE, wS, wSW), nrows, ncols, F,
              int(iter), float(omega), int(mode))


def oflow_res_elin4(RU, RV, U, V, M, Cu, Cv, Du, Dv, wW, wN, wE, wS):
    _chk(RU, RV, U, V, M, Cu, Cv, Du, Dv, wW, wN, wE, wS)
    nrows, ncols, _ = _dims(U)
    capi.call("pdeip_oflow_res_elin4_dev", _stream(), *_p(RU, RV, U, V, M, Cu, Cv, Du, Dv, wW, wN, wE, wS), nrows,
              ncols, _dims(M)[2])


def oflow_lhs_elin4(AU, AV, U, V, M, Du, Dv, wW, wN, wE, wS):
    _chk(AU, AV, U, V, M, Du, Dv, wW, wN, wE, wS)
    nrows, ncols, _ = _dims(U)
    capi.call("pdeip_oflow_lhs_elin4_dev", _stream(), *_p(AU, AV, U, V, M, Du, Dv, wW, wN, wE, wS), nrows, ncols,
              _dims(M)[2])


def diffweights6(D, eps, wW, wN, wE, wS):
    _chk(D, wW, wN, wE, wS)
    nrows, ncols, F = _dims(D)
    capi.call("pdeip_diffweights6_dev", _stream(), D.data_ptr(), nrows, ncols, F, float(eps), *_p(wW, wN, wE, wS))


def warp_bilinear(Iin, X, Y, Iout):
    _chk(Iin, X, Y, Iout)
    nrows, ncols, F = _dims(Iin)
    capi.call("pdeip_warp_bilinear_dev", _stream(), *_p(Iin, X, Y), nrows, ncols, F, Iout.data_ptr())


def ac_solver(PHI, D, GradNorm, Diff, tau, nu, out):
    """out = one AOS step of the geodesic active contour (AC_solver_2d); `out` must not alias an input."""
    _chk(PHI, D, GradNorm, Diff, out)
    nrows, ncols, F = _dims(PHI)
    capi.call("pdeip_ac_solver_dev", _stream(), *_p(PHI, D, GradNorm, Diff), nrows, ncols, F, float(tau), float(nu), out.data_ptr())


def reinit(PHI, T, out):
    """out = Reinit(PHI, T): the re-initialisation steps of t = 0:0.25:T (PHI is not modified)."""
    _chk(PHI, out)
    nrows, ncols, F = _dims(PHI)
    capi.call("pdeip_reinit_dev", _stream(), PHI.data_ptr(), nrows, ncols, F, float(T), out.data_ptr())


def select_kth(x, k, out):
    """out[0] = the k-th smallest (1-based) element of x (any shape, all of it), NaN last: sort(x(:))(k).  out: one float32."""
    _chk(x, out)
    capi.call("pdeip_select_kth_dev", _stream(), x.data_ptr(), int(x.numel()), int(k), out.data_ptr())


def gac_stopping(I, lam, Igrad_out, g_out, lam_out):
    """Igrad, g and lambda of the GAC drivers (GAC_v10a.m:57-75) from the image planes I [(C,) ncols, nrows]; lam < 0 selects
    lambda as the drivers do.  Igrad_out, g_out: planes [ncols, nrows]; lam_out: one float32."""
    _chk(I, Igrad_out, g_out, lam_out)
    nrows, ncols, C = _dims(I)
    capi.call("pdeip_gac_stopping_dev", _stream(), I.data_ptr(), nrows, ncols, C, float(lam), *_p(Igrad_out, g_out, lam_out))


def cv_solver(PHI, D, DH, GradNorm, tau, nu, out):
    """out = one AOS step of the Chan-Vese model (CV_solver_2d); `out` must not alias an input."""
    _chk(PHI, D, DH, GradNorm, out)
    nrows, ncols, F = _dims(PHI)
    capi.call("pdeip_cv_solver_dev", _stream(), *_p(PHI, D, DH, GradNorm), nrows, ncols, F, float(tau), float(nu), out.data_ptr())


def cv_terms(PHI, c0, c1, dh_floor, DH_out, G_out):
    """DH_out = 1/(pi*(c0 + PHI^2/c1)) floored at dh_floor (NaN: no floor), G_out = |grad PHI| (the segmentation drivers' terms)."""
    _chk(PHI, DH_out, G_out)
    nrows, ncols, F = _dims(PHI)
    capi.call("pdeip_cv_terms_dev", _stream(), PHI.data_ptr(), nrows, ncols, F, float(c0), float(c1), float(dh_floor),
              DH_out.data_ptr(), G_out.data_ptr())


def surface_fit_masked(PHI, D, order, M_in, err_thr, min_set_size, iter, M_out, dist_out=None, ndata_out=None, seed=0, sets=None):
    """The RANSAC surface fit on the pixels with PHI >= 0 (pdeip_surface_fit_masked_dev): PHI, D planes [ncols, nrows]; order 1 | 2;
    M_in float32 [3 | 6] tensor or None; M_out float32 [3 | 6]; dist_out a plane or None; ndata_out an int32 tensor of one element
    or None; sets an int32 tensor [iter, ncoef + 1] of 0-based ranks or None (then drawn from seed).  Nothing is read back."""
    _chk(PHI, D, M_out, *[t for t in (M_in, dist_out) if t is not None])
    if D.shape != PHI.shape or PHI.dim() != 2 or (dist_out is not None and dist_out.shape != PHI.shape):
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "surface_fit_masked: PHI, D and dist_out must be planes of one size")
    ncoef = 3 if order == 1 else 6
    if M_out.numel() != ncoef or (M_in is not None and M_in.numel() != ncoef):
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "surface_fit_masked: M_in and M_out must have %d elements" % ncoef)
    for t, n in ((ndata_out, 1), (sets, max(int(iter), 0) * (ncoef + 1))):
        if t is not None and (t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous() or t.numel() != n):
            raise capi.PdeipError(capi.PDEIP_ERR_ARG, "surface_fit_masked: ndata_out / sets must be contiguous int32 CUDA tensors of 1 / iter*(ncoef+1) elements")
    nrows, ncols, _ = _dims(PHI)
    opt = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    capi.call("pdeip_surface_fit_masked_dev", _stream(), PHI.data_ptr(), D.data_ptr(), nrows, ncols, int(order), opt(M_in), float(err_thr),
              float(min_set_size), int(iter), opt(sets), ctypes.c_ulonglong(int(seed) & ((1 << 64) - 1)), M_out.data_ptr(), opt(dist_out),
              opt(ndata_out))


def surface_fit_masked_batch(PHI, D, order, M_in, err_thr, min_set_size, iter, M_out, dist_out=None, ndata_out=None, seed=0, seed_stride=65536):
    """surface_fit_masked of S planes PHI [S, ncols, nrows] over one data plane D [ncols, nrows] in one chain of launches
    (pdeip_surface_fit_masked_batch_dev): segment s draws from seed + seed_stride*s.  M_in float32 [S, 3 | 6] or None; M_out
    float32 [S, 3 | 6] (may be M_in); dist_out [S, ncols, nrows] or None; ndata_out an int32 tensor of S elements or None.
    Nothing is read back."""
    _chk(PHI, D, M_out, *[t for t in (M_in, dist_out) if t is not None])
    if PHI.dim() != 3 or D.dim() != 2 or D.shape != PHI.shape[1:] or (dist_out is not None and dist_out.shape != PHI.shape):
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "surface_fit_masked_batch: PHI and dist_out must be [S, ncols, nrows], D one plane of that size")
    nrows, ncols, S = _dims(PHI)
    ncoef = 3 if order == 1 else 6
    if M_out.numel() != S * ncoef or (M_in is not None and M_in.numel() != S * ncoef):
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "surface_fit_masked_batch: M_in and M_out must have S x %d elements" % ncoef)
    if ndata_out is not None and (ndata_out.dtype != torch.int32 or not ndata_out.is_cuda or not ndata_out.is_contiguous() or ndata_out.numel() != S):
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "surface_fit_masked_batch: ndata_out must be a contiguous int32 CUDA tensor of S elements")
    opt = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    m64 = (1 << 64) - 1
    capi.call("pdeip_surface_fit_masked_batch_dev", _stream(), PHI.data_ptr(), D.data_ptr(), nrows, ncols, S, int(order), opt(M_in),
              float(err_thr), float(min_set_size), int(iter), ctypes.c_ulonglong(int(seed) & m64), ctypes.c_ulonglong(int(seed_stride) & m64),
              M_out.data_ptr(), opt(dist_out), opt(ndata_out))


class Diffusion4Params(ctypes.Structure):
    """pdeip_diffusion4_params: NaN keeps the driver's default (alpha 25, outer_iter 5)."""
    _fields_ = [("alpha", ctypes.c_double), ("outer_iter", ctypes.c_double)]


def diffusion4(I, alpha, outer_iter, out):
    """out = Diffusion4_v10(I, 'alpha', alpha, 'outer_iter', outer_iter) before its uint8 cast (NaN: the driver's default);
    `out` may be I itself (in place), otherwise I is not modified."""
    _chk(I, out)
    if out.shape != I.shape:
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "diffusion4: out is %s but I is %s" % (tuple(out.shape), tuple(I.shape)))
    nrows, ncols, C = _dims(I)
    prm = Diffusion4Params(float(alpha), float(outer_iter))
    capi.call("pdeip_diffusion4_dev", _stream(), I.data_ptr(), nrows, ncols, C, ctypes.addressof(prm), out.data_ptr())


# ---- structure-tensor anisotropic diffusion (csrc/pdeip_stensor.hip) ---------------------------------------

class Diffusion8Params(ctypes.Structure):
    """pdeip_diffusion8_params: every member a double, NaN keeps the default of the mode (include/pdeip.h)."""
    _fields_ = [(k, ctypes.c_double) for k in ("mode", "sigma", "rho", "lambda_", "alpha", "C", "tau", "iters", "inner_iter", "omega", "solver")]


_D8_KEYS = {k: k for k, _ in Diffusion8Params._fields_ if k not in ("mode", "lambda_")}
_D8_KEYS.update({"lambda": "lambda_", "lambda_": "lambda_"})
_D8_MODES = {"eed": 0.0, "ced": 1.0}


def diffusion8_params(mode="ced", who="diffusion8", **param):
    """The parameter struct of a mode ('eed' | 'ced') with the named members set (lambda: pass **{"lambda": v} or lambda_=v)."""
    if mode not in _D8_MODES:
        raise ValueError("%s: mode must be 'eed' or 'ced' (got %r)" % (who, mode))
    prm = Diffusion8Params(*([float("nan")] * len(Diffusion8Params._fields_)))
    prm.mode = _D8_MODES[mode]
    for k, v in param.items():
        if k not in _D8_KEYS:
            raise TypeError("%s: unknown parameter %r" % (who, k))
        setattr(prm, _D8_KEYS[k], float(v))
    return prm


def gauss_taps(sigma):
    """(taps as a float32 numpy array of 2R + 1, R) of pdeip_gauss_taps: host only."""
    buf = (ctypes.c_float * 65)()
    R = ctypes.c_int(-1)
    capi.call("pdeip_gauss_taps", float(sigma), ctypes.addressof(buf), 65, ctypes.byref(R))
    return np.array(buf[:2 * R.value + 1], dtype=np.float32), R.value


def gaussian(I, sigma, out=None):
    """out = G_sigma * I, separable, 'replicate' border, per plane of I [(F,) ncols, nrows]; out must not be I."""
    _chk(I)
    out = torch.empty_like(I) if out is None else out
    _chk(out)
    if out.shape != I.shape:
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "gaussian: out is %s but I is %s" % (tuple(out.shape), tuple(I.shape)))
    nrows, ncols, F = _dims(I)
    capi.call("pdeip_gauss_dev", _stream(), I.data_ptr(), nrows, ncols, F, float(sigma), out.data_ptr())
    return out


def structure_tensor(I, sigma, rho, J):
    """J [3, ncols, nrows] = G_rho * (sum over the channels of grad(v) grad(v)'), v = G_sigma * I: J11, J12, J22."""
    _chk(I, J)
    nrows, ncols, C = _dims(I)
    if tuple(J.shape) != (3, ncols, nrows):
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "structure_tensor: J is %s, not %s" % (tuple(J.shape), (3, ncols, nrows)))
    capi.call("pdeip_structure_tensor_dev", _stream(), I.data_ptr(), nrows, ncols, C, float(sigma), float(rho), J.data_ptr())


def st_weights(J, params, tau, TRACE, w8):
    """TRACE [ncols, nrows] and w8 [8, ncols, nrows] (W NW N NE E SE S SW, times tau) of the diffusion tensor of J; params: a
    Diffusion8Params (diffusion8_params) of which mode, lambda, alpha and C are read."""
    _chk(J, TRACE, w8)
    nrows, ncols, _ = _dims(J)
    if tuple(J.shape) != (3, ncols, nrows) or tuple(TRACE.shape) != (ncols, nrows) or tuple(w8.shape) != (8, ncols, nrows):
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "st_weights: J [3, ncols, nrows], TRACE [ncols, nrows] and w8 [8, ncols, nrows] expected")
    capi.call("pdeip_st_weights_dev", _stream(), J.data_ptr(), nrows, ncols, ctypes.addressof(params), float(tau), TRACE.data_ptr(), w8.data_ptr())


def st_weights_padded(J, params, tau, TRACE, w8):
    """st_weights onto planes with a one-pixel ring: TRACE [ncols + 2, nrows + 2], w8 [8, ncols + 2, nrows + 2]; TRACE = 1 and the
    weights 0 on the ring (what a PDEsolver8 call on the image inside its ring takes: include/pdeip.h)."""
    _chk(J, TRACE, w8)
    nrows, ncols, _ = _dims(J)
    if tuple(J.shape) != (3, ncols, nrows) or tuple(TRACE.shape) != (ncols + 2, nrows + 2) or tuple(w8.shape) != (8, ncols + 2, nrows + 2):
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "st_weights_padded: J [3, ncols, nrows], TRACE [ncols+2, nrows+2] and w8 [8, ncols+2, nrows+2] expected")
    capi.call("pdeip_st_weights_padded_dev", _stream(), J.data_ptr(), nrows, ncols, ctypes.addressof(params), float(tau), TRACE.data_ptr(),
              w8.data_ptr())


def st_pad(I, out, out2=None):
    """out (and out2) [(F,) ncols + 2, nrows + 2] = I inside a one-pixel ring of its nearest pixels."""
    _chk(I, out, *(() if out2 is None else (out2,)))
    nrows, ncols, F = _dims(I)
    want = tuple(I.shape[:-2]) + (ncols + 2, nrows + 2)
    if tuple(out.shape) != want or (out2 is not None and tuple(out2.shape) != want):
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "st_pad: the outputs must be %s" % (want,))
    capi.call("pdeip_st_pad_dev", _stream(), I.data_ptr(), nrows, ncols, F, out.data_ptr(), None if out2 is None else out2.data_ptr())


def st_crop(Ip, out):
    """out [(F,) ncols, nrows] = the inside of Ip [(F,) ncols + 2, nrows + 2]."""
    _chk(Ip, out)
    nrows, ncols, F = _dims(out)
    if tuple(Ip.shape) != tuple(out.shape[:-2]) + (ncols + 2, nrows + 2):
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "st_crop: Ip is %s for an output of %s" % (tuple(Ip.shape), tuple(out.shape)))
    capi.call("pdeip_st_crop_dev", _stream(), Ip.data_ptr(), nrows, ncols, F, out.data_ptr())


def diffusion8(I, params, out):
    """out = the EED / CED filtered I (pdeip_diffusion8_dev) in the library's current ordering; `out` may be I itself."""
    _chk(I, out)
    if out.shape != I.shape:
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "diffusion8: out is %s but I is %s" % (tuple(out.shape), tuple(I.shape)))
    nrows, ncols, C = _dims(I)
    capi.call("pdeip_diffusion8_dev", _stream(), I.data_ptr(), nrows, ncols, C, ctypes.addressof(params), out.data_ptr())


def fst_derivatives5(It0, It1, Idt, Idx, Idy):
    _chk(It0, It1, Idt, Idx, Idy)
    nrows, ncols, F = _dims(It0)
    capi.call("pdeip_fst_derivatives5_dev", _stream(), *_p(It0, It1), nrows, ncols, F, *_p(Idt, Idx, Idy))


def snd_derivatives5(It0, It1, Idxt, Idyt, Idxx, Idyy, Idxy):
    _chk(It0, It1, Idxt, Idyt, Idxx, Idyy, Idxy)
    nrows, ncols, F = _dims(It0)
    capi.call("pdeip_snd_derivatives5_dev", _stream(), *_p(It0, It1), nrows, ncols, F, *_p(Idxt, Idyt, Idxx, Idyy, Idxy))


# ---- MATLAB-side stages of a late-linearisation pyramid level (csrc/pdeip_flow.hpp) ----------------------

def flow_coords(U, V, X, Y):
    _chk(U, V, X, Y)
    nrows, ncols, _ = _dims(U)
    capi.call("pdeip_flow_coords_dev", _stream(), *_p(U, V), nrows, ncols, *_p(X, Y))


def flow_warp(U, V, I1, W1, I2=None, W2=None):
    """W1 = warp(I1) and optionally W2 = warp(I2) at (X+U, Y+V) in one launch (flow_coords + warp_bilinear x 2).
    V = None: the disparity drivers' warp along x only (Y = the row grid itself)."""
    _chk(U, I1, W1)
    v = None
    if V is not None:
        _chk(V)
        v = V.data_ptr()
    nrows, ncols, C1 = _dims(I1)
    if I2 is None:
        capi.call("pdeip_flow_warp_dev", _stream(), U.data_ptr(), v, I1.data_ptr(), C1, None, 0, nrows, ncols, W1.data_ptr(), None)
    else:
        _chk(I2, W2)
        capi.call("pdeip_flow_warp_dev", _stream(), U.data_ptr(), v, I1.data_ptr(), C1, I2.data_ptr(), _dims(I2)[2], nrows, ncols, *_p(W1, W2))


def flow_assemble(term1, term2, dU, dV, alpha, MGd, CuGd, CvGd, DuGd, DvGd):
    """term = (It, Ix, Iy, b) with [C, ncols, nrows] derivative arrays; term2 may be None, or the gradient-magnitude
    term (Ixt, Iyt, Ixx, Iyy, Ixy, b) built from snd_derivatives5."""
    It1, Ix1, Iy1, b1 = term1
    _chk(It1, Ix1, Iy1, dU, dV, MGd, CuGd, CvGd, DuGd, DvGd)
    nrows, ncols, C1 = _dims(It1)
    if term2 is not None and len(term2) == 6:
        _chk(*term2[:5])
        capi.call("pdeip_flow_assemble_gradmag_dev", _stream(), *_p(It1, Ix1, Iy1), C1, float(b1), *_p(*term2[:5]), _dims(term2[0])[2],
                  float(term2[5]), *_p(dU, dV), float(alpha), nrows, ncols, *_p(MGd, CuGd, CvGd, DuGd, DvGd))
        return
    if term2 is None:
        p2, C2, b2 = [None, None, None], 0, 0.0
    else:
        It2, Ix2, Iy2, b2 = term2
        _chk(It2, Ix2, Iy2)
        p2, C2 = _p(It2, Ix2, Iy2), _dims(It2)[2]
    capi.call("pdeip_flow_assemble_dev", _stream(), *_p(It1, Ix1, Iy1), C1, float(b1), *p2, C2, float(b2), *_p(dU, dV),
              float(alpha), nrows, ncols, *_p(MGd, CuGd, CvGd, DuGd, DvGd))


def flow_assemble_weights(term1, term2, U, V, dU, dV, alpha, MGd, CuGd, CvGd, DuGd, DvGd, wW, wN, wS, wE):
    """flow_assemble + flow_opdiffweights(U, V, dU, dV) in one launch (both only read the iterate)."""
    It1, Ix1, Iy1, b1 = term1
    _chk(It1, Ix1, Iy1, U, V, dU, dV, MGd, CuGd, CvGd, DuGd, DvGd, wW, wN, wS, wE)
    nrows, ncols, C1 = _dims(It1)
    if term2 is None:
        p2, C2, b2 = [None] * 5, 0, 0.0
    elif len(term2) == 6:
        _chk(*term2[:5])
        p2, C2, b2 = _p(*term2[:5]), _dims(term2[0])[2], term2[5]
    else:
        _chk(*term2[:3])
        p2, C2, b2 = _p(*term2[:3]) + [None, None], _dims(term2[0])[2], term2[3]
    capi.call("pdeip_flow_assemble_weights_dev", _stream(), *_p(It1, Ix1, Iy1), C1, float(b1), *p2, C2, float(b2), *_p(U, V, dU, dV),
              float(alpha), nrows, ncols, *_p(MGd, CuGd, CvGd, DuGd, DvGd, wW, wN, wS, wE))


def flow_opdiffweights(U, V, dU, dV, wW, wN, wS, wE):
    """dU = dV = None: OPdiffWeights(U, V)."""
    _chk(U, V, wW, wN, wS, wE) if dU is None else _chk(U, V, dU, dV, wW, wN, wS, wE)
    nrows, ncols, _ = _dims(U)
    d = [None, None] if dU is None else _p(dU, dV)
    capi.call("pdeip_flow_opdiffweights_dev", _stream(), *_p(U, V), *d, nrows, ncols, *_p(wW, wN, wS, wE))


def median3(A, B, out):
    """out = medfilt2(A + B, [3 3], 'symmetric'); B may be None."""
    _chk(A, out) if B is None else _chk(A, B, out)
    nrows, ncols, _ = _dims(A)
    capi.call("pdeip_median3_dev", _stream(), A.data_ptr(), None if B is None else B.data_ptr(), nrows, ncols, out.data_ptr())


def median3_pair(A0, B0, out0, A1, B1, out1):
    """out0 = medfilt2(A0 + B0), out1 = medfilt2(A1 + B1) in one launch; B0 / B1 may be None (out = medfilt2(A))."""
    _chk(*(t for t in (A0, B0, out0, A1, B1, out1) if t is not None))
    nrows, ncols, _ = _dims(A0)
    capi.call("pdeip_median3_pair_dev", _stream(), A0.data_ptr(), _ptr(B0), A1.data_ptr(), _ptr(B1), nrows, ncols, *_p(out0, out1))


def nanmedfilt2(A, out=None):
    """out = nanmedfilt2(A) of DispSegmentationSparse.m (colfilt(A, [3 3], 'sliding', @nanmedian): the NaN-ignoring 3x3 median with
    zero padding; pdeip_nanmedfilt2_dev): A [(F,) ncols, nrows], every plane on its own; out like A, not A itself.  Returns out."""
    if out is None:
        out = torch.empty_like(A)
    _chk(A, out)
    if out.shape != A.shape:
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "nanmedfilt2: out must have A's shape")
    nrows, ncols, F = _dims(A)
    capi.call("pdeip_nanmedfilt2_dev", _stream(), A.data_ptr(), nrows, ncols, F, out.data_ptr())
    return out


def disp_assemble(term1, term2, dU, alpha, CuGd, DuGd):
    """term = (It, Ix, b); term2 may be None (DispEminND_llin_2D.m:258-293) or the gradient-magnitude term (Ixt, Iyt, Ixx, Ixy, b)."""
    It1, Ix1, b1 = term1
    _chk(It1, Ix1, dU, CuGd, DuGd)
    nrows, ncols, C1 = _dims(It1)
    if term2 is not None and len(term2) == 5:
        _chk(*term2[:4])
        capi.call("pdeip_disp_assemble_gradmag_dev", _stream(), *_p(It1, Ix1), C1, float(b1), *_p(*term2[:4]), _dims(term2[0])[2],
                  float(term2[4]), dU.data_ptr(), float(alpha), nrows, ncols, *_p(CuGd, DuGd))
        return
    if term2 is None:
        p2, C2, b2 = [None, None], 0, 0.0
    else:
        It2, Ix2, b2 = term2
        _chk(It2, Ix2)
        p2, C2 = _p(It2, Ix2), _dims(It2)[2]
    capi.call("pdeip_disp_assemble_dev", _stream(), *_p(It1, Ix1), C1, float(b1), *p2, C2, float(b2), dU.data_ptr(), float(alpha),
              nrows, ncols, *_p(CuGd, DuGd))


def add(A, B, out):
    _chk(A, B, out)
    nrows, ncols, _ = _dims(A)
    capi.call("pdeip_add_dev", _stream(), *_p(A, B), nrows, ncols, out.data_ptr())


def tv_assemble(Iout, Iin, alpha, TRACE, B, w8):
    """TVdenoise8.m:80-86: ADdiffWeights(Iout), PsiData, TRACE, B; w8 = [aW, aNW, aN, aNE, aE, aSE, aS, aSW] (alpha-scaled)."""
    _chk(Iout, Iin, TRACE, B, *w8)
    nrows, ncols, F = _dims(Iout)
    capi.call("pdeip_tv_assemble_dev", _stream(), *_p(Iout, Iin), nrows, ncols, F, float(alpha), *_p(TRACE, B, *w8))


def hs_assemble(It0, It1, b1, b2, MGd, CuGd, CvGd, DuGd, DvGd):
    """FlowEminHS_elin_2D_v10.m:133-164: data terms of one scale from the frames [C, ncols, nrows] (or [ncols, nrows])."""
    _chk(It0, It1, MGd, CuGd, CvGd, DuGd, DvGd)
    nrows, ncols, C = _dims(It0)
    capi.call("pdeip_hs_assemble_dev", _stream(), *_p(It0, It1), C, float(b1), float(b2), nrows, ncols, *_p(MGd, CuGd, CvGd, DuGd, DvGd))


# ---- stages of the FAS full-multigrid flow driver (csrc/pdeip_fas.hpp) ------------------------------------

def _half(n):
    return (n + 1) // 2


def fas_gauss5(I, G):
    """imfilter(I, G, 'replicate', 'conv'); G: 5x5 numpy kernel."""
    import numpy as np
    _chk(I)
    nrows, ncols, F = _dims(I)
    g = np.asfortranarray(G, dtype=np.float32)
    out = torch.empty_like(I)
    capi.call("pdeip_fas_gauss5_dev", _stream(), I.data_ptr(), nrows, ncols, F, g.ctypes.data, out.data_ptr())
    return out


def fas_down(I):
    """[C, ncols, nrows] -> [C, ceil(ncols/2), ceil(nrows/2)] (lpf twice, 1:2:end)"""
    _chk(I)
    nrows, ncols, F = _dims(I)
    out = torch.empty(I.shape[:-2] + (_half(ncols), _half(nrows)), dtype=I.dtype, device=I.device)
    capi.call("pdeip_fas_down_dev", _stream(), I.data_ptr(), nrows, ncols, F, out.data_ptr())
    return out


def fas_prepare(It0, It1, b1, b2):
    """-> planes [13, C, ncols, nrows]: Idt, Idx, Idy, Idxx, Idyy, Idxy, Idxt, Idyt, M, Cu, Cv, Du, Dv"""
    _chk(It0, It1)
    nrows, ncols, F = _dims(It0)
    planes = torch.empty((13, F, ncols, nrows), dtype=It0.dtype, device=It0.device)
    capi.call("pdeip_fas_prepare_dev", _stream(), *_p(It0, It1), nrows, ncols, F, float(b1), float(b2), planes.data_ptr())
    return planes


def fas_assemble(planes, Cu, Cv, U, V, b1, b2, k, per_frame, MGd, CuGd, CvGd, DuGd, DvGd, gd=None):
    _chk(planes, U, V, MGd, DuGd, DvGd)
    nrows, ncols, _ = _dims(U)
    F = planes.shape[1]
    opt = lambda t: None if t is None else (_chk(t), t.data_ptr())[1]
    capi.call("pdeip_fas_assemble_dev", _stream(), planes.data_ptr(), opt(Cu), opt(Cv), *_p(U, V), nrows, ncols, F, float(b1),
              float(b2), float(k), int(bool(per_frame)), MGd.data_ptr(), opt(CuGd), opt(CvGd), DuGd.data_ptr(), DvGd.data_ptr(), opt(gd))


def fas_assemble_weights(planes, Cu, Cv, U, V, b1, b2, k, MGd, CuGd, CvGd, DuGd, DvGd, wW, wN, wS, wE):
    """fas_assemble(per_frame=False) + flow_opdiffweights(U, V, None, None) in one launch."""
    _chk(planes, U, V, MGd, DuGd, DvGd, wW, wN, wS, wE)
    nrows, ncols, _ = _dims(U)
    opt = lambda t: None if t is None else (_chk(t), t.data_ptr())[1]
    capi.call("pdeip_fas_assemble_weights_dev", _stream(), planes.data_ptr(), opt(Cu), opt(Cv), *_p(U, V), nrows, ncols, planes.shape[1],
              float(b1), float(b2), float(k), MGd.data_ptr(), opt(CuGd), opt(CvGd), DuGd.data_ptr(), DvGd.data_ptr(), *_p(wW, wN, wS, wE))


def fas_restrict(A, scale):
    _chk(A)
    nrows, ncols, F = _dims(A)
    out = torch.empty(A.shape[:-2] + (_half(ncols), _half(nrows)), dtype=A.dtype, device=A.device)
    capi.call("pdeip_fas_restrict_dev", _stream(), A.data_ptr(), nrows, ncols, F, float(scale), out.data_ptr())
    return out


def fas_rhs(R, A, gd):
    _chk(R, A, gd)
    nrows, ncols, F = _dims(R)
    out = torch.empty_like(R)
    capi.call("pdeip_fas_rhs_dev", _stream(), *_p(R, A, gd), nrows, ncols, F, out.data_ptr())
    return out


def fas_prolong_add(U, Uc, Ures, inv_scale):
    """In place on U."""
    _chk(U, Uc, Ures)
    nrows, ncols, _ = _dims(U)
    nrows_c, ncols_c, _ = _dims(Uc)
    capi.call("pdeip_fas_prolong_add_dev", _stream(), U.data_ptr(), nrows, ncols, *_p(Uc, Ures), nrows_c, ncols_c, float(inv_scale))


def fas_upscale(U, mul, nrows_out, ncols_out):
    """imresize(U.*mul, [nrows_out ncols_out]) (bicubic, enlarging) -> new [ncols_out, nrows_out] plane"""
    _chk(U)
    nrows, ncols, _ = _dims(U)
    out = torch.empty((ncols_out, nrows_out), dtype=U.dtype, device=U.device)
    capi.call("pdeip_fas_upscale_dev", _stream(), U.data_ptr(), nrows, ncols, float(mul), nrows_out, ncols_out, out.data_ptr())
    return out


def ad_weights(D, quantile, w8):
    """ADdiffWeights(D, quantile) of FlowEminAD_llin_2D_v10.m; w8 = [wW, wNW, wN, wNE, wE, wSE, wS, wSW] planes [ncols, nrows]."""
    _chk(D, *w8)
    nrows, ncols, F = _dims(D)
    capi.call("pdeip_ad_weights_dev", _stream(), D.data_ptr(), nrows, ncols, F, float(quantile), *_p(*w8))


def tv4_assemble(Iout, Iin, alpha, TRACE, B, w4):
    """TVdenoise4.m:84-98: DiffWeights(Iout), PsiData, TRACE, B; w4 = [aW, aN, aE, aS] (alpha-scaled)."""
    _chk(Iout, Iin, TRACE, B, *w4)
    nrows, ncols, F = _dims(Iout)
    capi.call("pdeip_tv4_assemble_dev", _stream(), *_p(Iout, Iin), nrows, ncols, F, float(alpha), *_p(TRACE, B, *w4))


def rgb2grad(I):
    """[C, ncols, nrows] (or [ncols, nrows]) -> [2C, ncols, nrows]: the x / y differences of every frame (fstTerm 'grad')."""
    _chk(I)
    nrows, ncols, F = _dims(I)
    out = torch.empty((2 * F, ncols, nrows), dtype=I.dtype, device=I.device)
    capi.call("pdeip_rgb2grad_dev", _stream(), I.data_ptr(), nrows, ncols, F, out.data_ptr())
    return out


# ---- symmetric stereo driver (csrc/pdeip_sym.hpp); float64 planes are MATLAB doubles ----------------------

def _chk64(*tensors):
    for t in tensors:
        if t.dtype != torch.float64 or not t.is_contiguous() or not t.is_cuda:
            raise capi.PdeipError(capi.PDEIP_ERR_ARG, "expected contiguous float64 CUDA tensors")


def disp_sor_llin_sym4(U0, dU0, Cu0, Du0, w0, U1, dU1, Cu1, Du1, w1, iter, omega, solver, mode=capi.MODE_EXACT_ORDER):
    """In place on dU0, dU1 (Disp_sor_llin_sym4_2d: GS_SOR_llinsym4_2d / GS_ALR_SOR_llinsym4_2d); w = [wW, wN, wE, wS]."""
    _chk(U0, dU0, Cu0, Du0, *w0, U1, dU1, Cu1, Du1, *w1)
    nrows, ncols, _ = _dims(U0)
    capi.call("pdeip_disp_sor_llin_sym4_dev", _stream(), *_p(U0, dU0, Cu0, Du0, *w0, U1, dU1, Cu1, Du1, *w1), nrows, ncols, int(iter),
              float(omega), int(solver), int(mode), 0)


def sym_warp_flow(U, Uq):
    """interp2(X, Y, U, X+Uq, Y) -> float64 plane"""
    _chk(U, Uq)
    nrows, ncols, _ = _dims(U)
    out = torch.empty(U.shape, dtype=torch.float64, device=U.device)
    capi.call("pdeip_sym_warp_flow_dev", _stream(), *_p(U, Uq), nrows, ncols, out.data_ptr())
    return out


def sym_flow_terms(U, Uw):
    """-> (Udt, Udx, CuS, DuS) float64 planes"""
    _chk(U)
    _chk64(Uw)
    nrows, ncols, _ = _dims(U)
    outs = [torch.empty_like(Uw) for _ in range(4)]
    capi.call("pdeip_sym_flow_terms_dev", _stream(), U.data_ptr(), Uw.data_ptr(), nrows, ncols, *_p(*outs))
    return outs


def sym_assemble(d, sym, dU, b1, b2, alpha, kS, sr2, first, CuG, DuG):
    """d = (Idt, Idx, Idxt, Idyt, Idxx, Idxy) [C, ncols, nrows]; sym = (Udt, Udx, CuS, DuS) float64."""
    _chk(*d, dU, CuG, DuG)
    _chk64(*sym)
    nrows, ncols, C = _dims(d[0])
    capi.call("pdeip_sym_assemble_dev", _stream(), *_p(*d), C, *_p(*sym), dU.data_ptr(), float(b1), float(b2), float(alpha), float(kS),
              float(sr2), int(bool(first)), nrows, ncols, *_p(CuG, DuG))


def flow_apriori(Us, U, dU, gammaS, alpha, as_diff, u_double, du_double, CGd, DGd):
    """Adds the spatial a-priori slice (FlowEminND_llin_2D_v10.m:301-325) to CGd / DGd in place; Us float64."""
    _chk(U, dU, CGd, DGd)
    _chk64(Us)
    nrows, ncols, _ = _dims(U)
    capi.call("pdeip_flow_apriori_dev", _stream(), Us.data_ptr(), U.data_ptr(), dU.data_ptr(), float(gammaS), float(alpha), float(as_diff),
              int(bool(u_double)), int(bool(du_double)), nrows, ncols, CGd.data_ptr(), DGd.data_ptr())


def disp_apriori(Us, U, dU, gammaS, alpha, as_diff, u_double, du_double, CGd, DGd):
    """Adds the disparity driver's spatial a-priori slice (DispEminND_llin_2D.m:277-292, exp influence function) to CGd / DGd."""
    _chk(U, dU, CGd, DGd)
    _chk64(Us)
    nrows, ncols, _ = _dims(U)
    capi.call("pdeip_disp_apriori_dev", _stream(), Us.data_ptr(), U.data_ptr(), dU.data_ptr(), float(gammaS), float(alpha), float(as_diff),
              int(bool(u_double)), int(bool(du_double)), nrows, ncols, CGd.data_ptr(), DGd.data_ptr())


# ---- the drivers' image pyramid on the device (csrc/pdeip_pyr.hpp; definitions in pyramid.py) -------------

def pyr_resize(I, nrows_out, ncols_out, method="bilinear"):
    """pyramid.resize on the device: [(C,) ncols, nrows] -> [(C,) ncols_out, nrows_out]"""
    _chk(I)
    nrows, ncols, F = _dims(I)
    out = torch.empty(I.shape[:-2] + (ncols_out, nrows_out), dtype=I.dtype, device=I.device)
    capi.call("pdeip_pyr_resize_dev", _stream(), I.data_ptr(), nrows, ncols, F, int(nrows_out), int(ncols_out), int(method == "bicubic"),
              out.data_ptr())
    return out


def pyr_smooth(I, G):
    """pyramid.smooth on the device; G: odd square numpy mask (float64)"""
    _chk(I)
    nrows, ncols, F = _dims(I)
    g = np.ascontiguousarray(G, dtype=np.float64)
    out = torch.empty_like(I)
    capi.call("pdeip_pyr_smooth_dev", _stream(), I.data_ptr(), nrows, ncols, F, g.ctypes.data, int(g.shape[0]), out.data_ptr())
    return out


# ---- region competition: the segmentation drivers' inner loop (csrc/pdeip_segmentation.hip; the contract: include/pdeip.h) ----

class SegParams(ctypes.Structure):
    """pdeip_seg_params: NaN keeps the dense driver's value; SegParams.sparse() is DispSegmentationSparse.m's form."""
    _fields_ = [(k, ctypes.c_double) for k in ("c0", "c1", "dh_floor", "err_thr", "gamma_coef", "dist_cap", "nan_fill")]

    @classmethod
    def make(cls, sparse=False, **param):
        vals = dict(c0=2.0, c1=4.0, dh_floor=0.04, err_thr=1.2, gamma_coef=0.005, dist_cap=100.0, nan_fill=1000.0) if sparse else {}
        for k, v in param.items():
            if k not in dict(cls._fields_):
                raise TypeError("unknown segmentation parameter %r" % k)
            vals[k] = float(v)
        return cls(*[vals.get(k, float("nan")) for k, _ in cls._fields_])


SEG_STRATEGIES = {"surface": capi.SEG_SURFACE, "greedy": capi.SEG_GREEDY, "inverse": capi.SEG_INVERSE}


def _strategy(competition):
    if competition not in SEG_STRATEGIES:
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "No such competition strategy! (%r)" % (competition,))
    return SEG_STRATEGIES[competition]


def _chk_typed(t, dtype, n, what):
    if t.dtype != dtype or not t.is_cuda or not t.is_contiguous() or t.numel() < n:
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "%s must be a contiguous %s CUDA tensor of at least %d elements" % (what, dtype, n))


def seg_sizes(PHI, sizes_out):
    """sizes_out[s] = #{PHI_s >= 0}: PHI [S, ncols, nrows], sizes_out int32 [S].  Nothing is read back."""
    _chk(PHI)
    nrows, ncols, S = _dims(PHI)
    _chk_typed(sizes_out, torch.int32, S, "seg_sizes: sizes_out")
    capi.call("pdeip_seg_sizes_dev", _stream(), PHI.data_ptr(), nrows, ncols, S, sizes_out.data_ptr())


def seg_variance(PHI, dist, minCOV, dist_cap, cov_out, n_out=None):
    """cov_out[s] = max(mean of dist over PHI_s >= 0 (and dist < dist_cap when that is finite), minCOV) in float64; cov_out float64
    [S], n_out int32 [S] or None."""
    _chk(PHI, dist)
    nrows, ncols, S = _dims(PHI)
    if dist.shape != PHI.shape:
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "seg_variance: dist must have PHI's shape")
    _chk_typed(cov_out, torch.float64, S, "seg_variance: cov_out")
    if n_out is not None:
        _chk_typed(n_out, torch.int32, S, "seg_variance: n_out")
    capi.call("pdeip_seg_variance_dev", _stream(), PHI.data_ptr(), dist.data_ptr(), nrows, ncols, S, float(minCOV), float(dist_cap),
              cov_out.data_ptr(), n_out.data_ptr() if n_out is not None else None)


def seg_data(dist, PHI, DH, cov, competition, DATA_out, P_out=None):
    """The likelihood, competitor and log-odds planes: DATA_out float32 like PHI; P_out float64 like PHI or None; cov float64 [S]."""
    _chk(dist, PHI, DH, DATA_out)
    nrows, ncols, S = _dims(PHI)
    if not (dist.shape == PHI.shape == DH.shape == DATA_out.shape):
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "seg_data: dist, PHI, DH and DATA_out must have one shape")
    _chk_typed(cov, torch.float64, S, "seg_data: cov")
    if P_out is not None:
        _chk_typed(P_out, torch.float64, PHI.numel(), "seg_data: P_out")
    capi.call("pdeip_seg_data_dev", _stream(), dist.data_ptr(), PHI.data_ptr(), DH.data_ptr(), cov.data_ptr(), nrows, ncols, S,
              _strategy(competition), DATA_out.data_ptr(), P_out.data_ptr() if P_out is not None else None)


def seg_competition_level(PHI, D, order, minCOV, ransac_cset, iterations, srem_thr, competition="inverse", seed=0, fit_counter=0, prm=None):
    """`iterations` competition iterations on one scale (pdeip_seg_competition_level_dev): PHI [S, ncols, nrows], D [ncols, nrows].
    Returns (PHI_out [S_out, ncols, nrows], surf [S_out, ncoef], kept (list of input indices), cov float64 [S_out], fit_counter
    after the call).  The call synchronises the stream once per iteration (the sizes decide removal on the host)."""
    _chk(PHI, D)
    if PHI.dim() != 3 or D.shape != PHI.shape[1:]:
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "seg_competition_level: PHI must be [S, ncols, nrows] and D [ncols, nrows]")
    nrows, ncols, S = _dims(PHI)
    ncoef = 6 if order == 2 else 3
    out = torch.empty_like(PHI)
    surf = torch.zeros((S, ncoef), dtype=torch.float32, device=PHI.device)
    cov = torch.zeros(S, dtype=torch.float64, device=PHI.device)
    s_out = ctypes.c_int(0)
    kept = (ctypes.c_int * S)()
    fit = ctypes.c_ulonglong(int(fit_counter))
    prm = prm if prm is not None else SegParams.make()
    capi.call("pdeip_seg_competition_level_dev", _stream(), PHI.data_ptr(), D.data_ptr(), nrows, ncols, S, int(order), _strategy(competition),
              float(minCOV), float(ransac_cset), int(iterations), float(srem_thr), ctypes.c_ulonglong(int(seed) & ((1 << 64) - 1)),
              ctypes.addressof(fit), ctypes.addressof(prm), ctypes.addressof(s_out), out.data_ptr(), surf.data_ptr(), ctypes.addressof(kept),
              cov.data_ptr())
    n = s_out.value
    return out[:n], surf[:n], [int(k) for k in kept[:n]], cov[:n], int(fit.value)


def seg_label(PHI, SEG_out=None):
    """The numbered map: sum of s*[PHI_s > 0] over 1-based s, 0 where segments overlap; int32 [ncols, nrows]."""
    _chk(PHI)
    nrows, ncols, S = _dims(PHI)
    if SEG_out is None:
        SEG_out = torch.empty(PHI.shape[-2:], dtype=torch.int32, device=PHI.device)
    _chk_typed(SEG_out, torch.int32, nrows * ncols, "seg_label: SEG_out")
    capi.call("pdeip_seg_label_dev", _stream(), PHI.data_ptr(), nrows, ncols, S, SEG_out.data_ptr())
    return SEG_out


def bwlabel(A, conn=8, L_out=None, num_out=None, areas_out=None):
    """[L, num] = bwlabel(A > 0, conn) with MATLAB's numbering (pdeip_bwlabel_dev): A float32 [ncols, nrows]; L_out int32 like A,
    num_out int32 [1], areas_out int32 [cap] or None (areas_out[l-1] = pixels of component l).  Returns (L_out, num_out, areas_out)
    as tensors; nothing is read back."""
    _chk(A)
    if A.dim() != 2:
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "bwlabel: A must be one plane [ncols, nrows]")
    nrows, ncols, _ = _dims(A)
    if L_out is None:
        L_out = torch.empty(A.shape, dtype=torch.int32, device=A.device)
    if num_out is None:
        num_out = torch.empty(1, dtype=torch.int32, device=A.device)
    _chk_typed(L_out, torch.int32, nrows * ncols, "bwlabel: L_out")
    _chk_typed(num_out, torch.int32, 1, "bwlabel: num_out")
    cap = 0
    if areas_out is not None:
        cap = int(areas_out.numel())
        _chk_typed(areas_out, torch.int32, cap, "bwlabel: areas_out")
    capi.call("pdeip_bwlabel_dev", _stream(), A.data_ptr(), nrows, ncols, int(conn), L_out.data_ptr(), num_out.data_ptr(),
              areas_out.data_ptr() if cap else None, cap)
    return L_out, num_out, areas_out


def largest_component(A, conn=8, hi=1.0, lo=0.0, out=None, num_out=None, area_out=None):
    """out = lo everywhere, hi on the largest component of A > 0 (the lowest label on a tie; pdeip_largest_component_dev).  out
    float32 like A (A itself is allowed); num_out / area_out int32 [1] or None.  Returns out."""
    _chk(A)
    if A.dim() != 2:
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "largest_component: A must be one plane [ncols, nrows]")
    nrows, ncols, _ = _dims(A)
    if out is None:
        out = torch.empty_like(A)
    _chk(out)
    if out.numel() != A.numel():
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "largest_component: out must have A's shape")
    for t, what in ((num_out, "num_out"), (area_out, "area_out")):
        if t is not None:
            _chk_typed(t, torch.int32, 1, "largest_component: " + what)
    capi.call("pdeip_largest_component_dev", _stream(), A.data_ptr(), nrows, ncols, int(conn), float(hi), float(lo), out.data_ptr(),
              num_out.data_ptr() if num_out is not None else None, area_out.data_ptr() if area_out is not None else None)
    return out


# ---- flow colour coding and error measures (csrc/pdeip_flowviz.hip) ----
def flow2color(U, V, maxvalue=None, border=0, uint8=False, out=None, maxvalue_out=None):
    """img = flow2color(cat(3, U, V), 'maxvalue', maxvalue, 'border', border) on resident planes (pdeip_flow2color_dev): U, V
    [ncols, nrows]; maxvalue None: the field's largest magnitude, found on the device.  Returns (img, maxvalue_out): img float32
    [3, bcols, brows] (MATLAB's [brows, bcols, 3]; to_matlab converts) or, with uint8=True, the uint8 tensor [brows, bcols, 3] an image
    writer takes; maxvalue_out a float64 tensor [1] holding the maximum used.  Nothing is read back."""
    _chk(U, V)
    if U.dim() != 2 or V.shape != U.shape:
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "flow2color: U and V must be planes [ncols, nrows] of one shape")
    nrows, ncols, _ = _dims(U)
    border = int(border)
    brows, bcols = nrows + 2 * max(border, 0), ncols + 2 * max(border, 0)
    if out is None:
        out = (torch.empty((brows, bcols, 3), dtype=torch.uint8, device=U.device) if uint8
               else torch.empty((3, bcols, brows), dtype=torch.float32, device=U.device))
    _chk_typed(out, torch.uint8 if uint8 else torch.float32, 3 * brows * bcols, "flow2color: out")
    if maxvalue_out is None:
        maxvalue_out = torch.empty(1, dtype=torch.float64, device=U.device)
    _chk_typed(maxvalue_out, torch.float64, 1, "flow2color: maxvalue_out")
    capi.call("pdeip_flow2color_dev", _stream(), U.data_ptr(), V.data_ptr(), nrows, ncols, float("nan") if maxvalue is None else float(maxvalue),
              border, None if uint8 else out.data_ptr(), out.data_ptr() if uint8 else None, maxvalue_out.data_ptr())
    return out, maxvalue_out


def flow_errors(U, V, Ut, Vt, mask=None, epe_out=None, ang_out=None, stats_out=None, planes=True):
    """Endpoint and angular error of the resident flow (U, V) against (Ut, Vt) (pdeip_flow_errors_dev); mask: a float32 plane,
    nonzero where a pixel counts, or None.  Returns (epe, ang, stats): the two error planes like U (NaN where a pixel does not
    count; None with planes=False) and a float64 tensor [4] = count, mean endpoint error, mean angular error in degrees, largest
    endpoint error.  Nothing is read back."""
    fields = (U, V, Ut, Vt) if mask is None else (U, V, Ut, Vt, mask)
    _chk(*fields)
    if U.dim() != 2 or any(t.shape != U.shape for t in fields):
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "flow_errors: U, V, Ut, Vt and mask must be planes [ncols, nrows] of one shape")
    nrows, ncols, _ = _dims(U)
    if planes:
        epe_out = torch.empty_like(U) if epe_out is None else epe_out
        ang_out = torch.empty_like(U) if ang_out is None else ang_out
    for t, what in ((epe_out, "epe_out"), (ang_out, "ang_out")):
        if t is not None:
            _chk_typed(t, torch.float32, nrows * ncols, "flow_errors: " + what)
    if stats_out is None:
        stats_out = torch.empty(4, dtype=torch.float64, device=U.device)
    _chk_typed(stats_out, torch.float64, 4, "flow_errors: stats_out")
    capi.call("pdeip_flow_errors_dev", _stream(), *_p(U, V, Ut, Vt), None if mask is None else mask.data_ptr(), nrows, ncols,
              None if epe_out is None else epe_out.data_ptr(), None if ang_out is None else ang_out.data_ptr(), stats_out.data_ptr())
    return epe_out, ang_out, stats_out


# ---- cross-checks (csrc/pdeip_crosscheck.hip) ----
def _out_plane(like, given, wanted, what):
    if given is None and wanted:
        given = torch.empty_like(like)
    if given is not None:
        _chk_typed(given, torch.float32, like.numel(), what)
    return given


def _ptr(t):
    return None if t is None else t.data_ptr()


def disp_crosscheck(D0, D1, tol=1.0, sparse_out=None, mask_out=None, diff_out=None, stats_out=None, planes=True):
    """The left-right check of the resident disparity D0 against the other view's D1 (pdeip_disp_crosscheck_dev), both [ncols, nrows].
    Returns (sparse, mask, diff, stats): D0 where kept and NaN elsewhere, 1 / 0, D0 + the sampled D1 (planes like D0; with
    planes=False only those handed in are written, the others are None) and a float64 tensor [4] = kept, defined, mean |diff|, largest
    |diff|.  sparse_out may be D0.  Nothing is read back."""
    _chk(D0, D1)
    if D0.dim() != 2 or D1.shape != D0.shape:
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "disp_crosscheck: D0 and D1 must be planes [ncols, nrows] of one shape")
    nrows, ncols, _ = _dims(D0)
    sparse_out = _out_plane(D0, sparse_out, planes, "disp_crosscheck: sparse_out")
    mask_out = _out_plane(D0, mask_out, planes, "disp_crosscheck: mask_out")
    diff_out = _out_plane(D0, diff_out, planes, "disp_crosscheck: diff_out")
    if stats_out is None:
        stats_out = torch.empty(4, dtype=torch.float64, device=D0.device)
    _chk_typed(stats_out, torch.float64, 4, "disp_crosscheck: stats_out")
    capi.call("pdeip_disp_crosscheck_dev", _stream(), *_p(D0, D1), nrows, ncols, float(tol), _ptr(sparse_out), _ptr(mask_out),
              _ptr(diff_out), stats_out.data_ptr())
    return sparse_out, mask_out, diff_out, stats_out


def flow_crosscheck(Uf, Vf, Ub, Vb, a=0.01, b=0.5, mask_out=None, err_out=None, stats_out=None, planes=True):
    """The forward-backward check of the resident flow (Uf, Vf) of frame 0 -> 1 against (Ub, Vb) of frame 1 -> 0
    (pdeip_flow_crosscheck_dev).  Returns (mask, err, stats): 1 / 0, |f + b(x + f)| (planes like Uf; None with planes=False unless
    handed in) and a float64 tensor [4] = kept, defined, mean err, largest err.  mask is what flow_errors takes.  Nothing is read back."""
    _chk(Uf, Vf, Ub, Vb)
    if Uf.dim() != 2 or any(t.shape != Uf.shape for t in (Vf, Ub, Vb)):
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "flow_crosscheck: Uf, Vf, Ub and Vb must be planes [ncols, nrows] of one shape")
    nrows, ncols, _ = _dims(Uf)
    mask_out = _out_plane(Uf, mask_out, planes, "flow_crosscheck: mask_out")
    err_out = _out_plane(Uf, err_out, planes, "flow_crosscheck: err_out")
    if stats_out is None:
        stats_out = torch.empty(4, dtype=torch.float64, device=Uf.device)
    _chk_typed(stats_out, torch.float64, 4, "flow_crosscheck: stats_out")
    capi.call("pdeip_flow_crosscheck_dev", _stream(), *_p(Uf, Vf, Ub, Vb), nrows, ncols, float(a), float(b), _ptr(mask_out), _ptr(err_out),
              stats_out.data_ptr())
    return mask_out, err_out, stats_out


# ---- hole filling: TV inpainting of a sparse map (csrc/pdeip_inpaint.hip) ----
class InpaintParams(ctypes.Structure):
    """pdeip_inpaint_params: a member <= 0 keeps the driver's default; keep: 0 no merge, 1 merge."""
    _fields_ = [(k, ctypes.c_double) for k in ("alpha", "omega", "scl_factor", "cover", "guide_scale")] + \
               [(k, ctypes.c_int) for k in ("outer_iter", "inner_iter", "solver", "min_size", "keep")]

    @classmethod
    def make(cls, **param):
        s = cls(keep=-1)
        for k, v in param.items():
            if k not in dict(cls._fields_):
                raise capi.PdeipError(capi.PDEIP_ERR_ARG, "tv_inpaint4: unknown parameter '%s'" % k)
            setattr(s, k, type(getattr(s, k))(v))
        return s


def _guide(like, guide, who):
    """(pointer, channels) of an optional guide [(C,) ncols, nrows] on the frame of `like`."""
    if guide is None:
        return None, 0
    _chk(guide)
    if guide.shape[-2:] != like.shape[-2:]:
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "%s: the guide is %s but the map is %s" % (who, tuple(guide.shape), tuple(like.shape)))
    return guide.data_ptr(), _dims(guide)[2]


def nan_resize(D, nrows_out, ncols_out, cover=0.25):
    """The NaN-aware pyramid.resize (bilinear): [(F,) ncols, nrows] -> [(F,) ncols_out, nrows_out]; a pixel whose known taps weigh
    less than `cover` is NaN."""
    _chk(D)
    nrows, ncols, F = _dims(D)
    out = torch.empty(D.shape[:-2] + (int(ncols_out), int(nrows_out)), dtype=D.dtype, device=D.device)
    capi.call("pdeip_nan_resize_dev", _stream(), D.data_ptr(), nrows, ncols, F, int(nrows_out), int(ncols_out), float(cover), out.data_ptr())
    return out


def inpaint_meanfill(D, out=None):
    """Holes (NaN) take the mean of their frame's known values, known pixels keep their bits."""
    _chk(D)
    out = torch.empty_like(D) if out is None else out
    _chk_typed(out, torch.float32, D.numel(), "inpaint_meanfill: out")
    nrows, ncols, F = _dims(D)
    capi.call("pdeip_inpaint_meanfill_dev", _stream(), D.data_ptr(), nrows, ncols, F, out.data_ptr())
    return out


def tv4_inpaint_assemble(X, D, alpha, TRACE, B, w4, guide=None, guide_scale=20.0):
    """tv4_assemble for a sparse D: NaN TRACE and zero B on holes, the weights' maximum also over guide_scale * guide;
    w4 = [aW, aN, aE, aS]."""
    _chk(X, D, TRACE, B, *w4)
    if any(t.shape != X.shape for t in (D, TRACE, B, *w4)):
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "tv4_inpaint_assemble: X, D, TRACE, B and the weights must have one shape")
    gp, gc = _guide(X, guide, "tv4_inpaint_assemble")
    nrows, ncols, F = _dims(X)
    capi.call("pdeip_tv4_inpaint_assemble_dev", _stream(), *_p(X, D), gp, gc, float(guide_scale), nrows, ncols, F, float(alpha),
              *_p(TRACE, B, *w4))


def inpaint_merge(X, D, out=None, filled_out=None):
    """out = D where D is a number (its own bits), X elsewhere; filled_out (optional) = 1 on holes.  Returns out."""
    _chk(X, D)
    if D.shape != X.shape:
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "inpaint_merge: X and D must have one shape")
    out = torch.empty_like(X) if out is None else out
    _chk_typed(out, torch.float32, X.numel(), "inpaint_merge: out")
    if filled_out is not None:
        _chk_typed(filled_out, torch.float32, X.numel(), "inpaint_merge: filled_out")
    nrows, ncols, F = _dims(X)
    capi.call("pdeip_inpaint_merge_dev", _stream(), *_p(X, D), nrows, ncols, F, out.data_ptr(), _ptr(filled_out))
    return out


def tv_inpaint4(D, guide=None, out=None, filled_out=None, mode=None, **param):
    """The whole resident run (pdeip_tv_inpaint4_dev): D [(F,) ncols, nrows] with NaN holes, guide [(C,) ncols, nrows] or None.
    Returns out (a plane like D).  mode: the ordering of the solver calls (None: the library's current mode).  Nothing is read back."""
    _chk(D)
    gp, gc = _guide(D, guide, "tv_inpaint4")
    out = torch.empty_like(D) if out is None else out
    _chk_typed(out, torch.float32, D.numel(), "tv_inpaint4: out")
    if filled_out is not None:
        _chk_typed(filled_out, torch.float32, D.numel(), "tv_inpaint4: filled_out")
    nrows, ncols, F = _dims(D)
    prm = InpaintParams.make(**param)
    old = capi.get_mode()
    if mode is not None:
        capi.set_mode(mode)
    try:
        capi.call("pdeip_tv_inpaint4_dev", _stream(), D.data_ptr(), nrows, ncols, F, gp, gc, ctypes.addressof(prm), out.data_ptr(),
                  _ptr(filled_out))
    finally:
        if mode is not None:
            capi.set_mode(old)
    return out


# ---- frame interpolation from a computed flow (csrc/pdeip_interp.hip) ----
class InterpParams(ctypes.Structure):
    """pdeip_interp_params: a, b the cross-checks' thresholds, use_costs 0 = the lowest index wins a target, fill the hole filling's
    parameters (InpaintParams; kept alive by this object).  Any other keyword goes to the hole filling."""
    _fields_ = [("a", ctypes.c_double), ("b", ctypes.c_double), ("use_costs", ctypes.c_int), ("fill", ctypes.c_void_p)]

    @classmethod
    def make(cls, **param):
        s = cls(a=0.01, b=0.5, use_costs=1, fill=None)
        for k in ("a", "b", "use_costs"):
            if k in param:
                setattr(s, k, type(getattr(s, k))(param.pop(k)))
        s._fill = None
        if param:
            try:
                s._fill = InpaintParams.make(**param)
            except capi.PdeipError as exc:
                raise capi.PdeipError(exc.code, str(exc).replace("tv_inpaint4", "flow_interpolate")) from None
            s.fill = ctypes.addressof(s._fill)
        return s


def _images(I0, I1, like, who):
    """Channels of the two frames [(C,) ncols, nrows] on the frame of `like`."""
    _chk(I0, I1)
    if I0.shape != I1.shape or I0.shape[-2:] != like.shape[-2:]:
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "%s: the frames are %s and %s but the flow is %s"
                              % (who, tuple(I0.shape), tuple(I1.shape), tuple(like.shape)))
    return _dims(I0)[2]


def _flow_planes(who, first, *rest):
    fields = (first,) + tuple(t for t in rest if t is not None)
    _chk(*fields)
    if first.dim() != 2 or any(t.shape != first.shape for t in fields):
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "%s: the flow and mask planes must be planes [ncols, nrows] of one shape" % who)


def flow_splat(Uf, Vf, t=0.5, I0=None, I1=None, Ut_out=None, Vt_out=None, cost_out=None, cost=True):
    """The resident flow (Uf, Vf) of frame 0 -> 1 carried forward to time t (pdeip_flow_splat_dev): every target takes the source
    of the lowest photo-consistency cost |I0 - I1(x + f)| (frames [(C,) ncols, nrows]; without frames the lowest index).  Returns
    (Ut, Vt, cost): NaN where nothing landed; cost None with cost=False unless handed in.  Nothing is read back."""
    _flow_planes("flow_splat", Uf, Vf)
    if (I0 is None) != (I1 is None):
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "flow_splat: I0 and I1 must both be given or both be None")
    channels = 0 if I0 is None else _images(I0, I1, Uf, "flow_splat")
    nrows, ncols, _ = _dims(Uf)
    Ut_out = _out_plane(Uf, Ut_out, True, "flow_splat: Ut_out")
    Vt_out = _out_plane(Uf, Vt_out, True, "flow_splat: Vt_out")
    cost_out = _out_plane(Uf, cost_out, cost, "flow_splat: cost_out")
    capi.call("pdeip_flow_splat_dev", _stream(), *_p(Uf, Vf), _ptr(I0), _ptr(I1), channels, nrows, ncols, float(t), *_p(Ut_out, Vt_out),
              _ptr(cost_out))
    return Ut_out, Vt_out, cost_out


def interp_blend(I0, I1, Ut, Vt, t=0.5, M0=None, M1=None, It_out=None, source_out=None, source=True):
    """The picture at time t along the dense resident flow (Ut, Vt) given at t (pdeip_interp_blend_dev); M0, M1: the masks of
    flow_crosscheck for the forward flow in frame 0 and the backward flow in frame 1, or None.  Returns (It, source): It like I0,
    source 0 neither frame, 1 frame 0, 2 frame 1, 3 both (None with source=False unless handed in).  Nothing is read back."""
    _flow_planes("interp_blend", Ut, Vt, M0, M1)
    if (M0 is None) != (M1 is None):
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "interp_blend: M0 and M1 must both be given or both be None")
    channels = _images(I0, I1, Ut, "interp_blend")
    nrows, ncols, _ = _dims(Ut)
    It_out = _out_plane(I0, It_out, True, "interp_blend: It_out")
    source_out = _out_plane(Ut, source_out, source, "interp_blend: source_out")
    capi.call("pdeip_interp_blend_dev", _stream(), *_p(I0, I1), channels, *_p(Ut, Vt), _ptr(M0), _ptr(M1), nrows, ncols, float(t),
              It_out.data_ptr(), _ptr(source_out))
    return It_out, source_out


def flow_interpolate(I0, I1, Uf, Vf, Ub=None, Vb=None, t=0.5, It_out=None, Ut_out=None, Vt_out=None, source_out=None, flow=True, source=True,
                     mode=None, fill_with="tv", max_dist=0, **param):
    """The whole resident chain (pdeip_flow_interpolate_dev): the cross-checks of (Uf, Vf) against (Ub, Vb) if the backward flow is
    given, the splat to time t, the hole filling and the blend.  Returns (It, Ut, Vt, source): the frame at t like I0, the filled flow
    at t and the source plane (None with flow=False / source=False unless handed in).  mode: the ordering of the hole filling's solver
    calls (None: the library's current mode); param: a, b, use_costs and tv_inpaint4's.  fill_with="nearest": the holes take the
    nearest source's flow instead (pdeip_flow_interpolate_nearest_dev; max_dist > 0 fills only that far, the rest becomes 0); TV
    parameters are then a ValueError.  Nothing is read back."""
    if fill_with not in ("tv", "nearest"):
        raise ValueError("flow_interpolate: fill_with must be 'tv' or 'nearest' (got %r)" % (fill_with,))
    if fill_with == "nearest":
        tv = sorted(k for k in param if k not in ("a", "b", "use_costs"))
        if tv:
            raise ValueError("flow_interpolate: fill_with='nearest' takes no TV inpainting parameters (got %s)" % tv)
    elif max_dist:
        raise ValueError("flow_interpolate: max_dist belongs to fill_with='nearest'")
    _flow_planes("flow_interpolate", Uf, Vf, Ub, Vb)
    if (Ub is None) != (Vb is None):
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "flow_interpolate: Ub and Vb must both be given or both be None")
    channels = _images(I0, I1, Uf, "flow_interpolate")
    nrows, ncols, _ = _dims(Uf)
    It_out = _out_plane(I0, It_out, True, "flow_interpolate: It_out")
    Ut_out = _out_plane(Uf, Ut_out, flow, "flow_interpolate: Ut_out")
    Vt_out = _out_plane(Uf, Vt_out, flow, "flow_interpolate: Vt_out")
    source_out = _out_plane(Uf, source_out, source, "flow_interpolate: source_out")
    prm = InterpParams.make(**param)
    if fill_with == "nearest":
        capi.call("pdeip_flow_interpolate_nearest_dev", _stream(), *_p(I0, I1), channels, *_p(Uf, Vf), _ptr(Ub), _ptr(Vb), nrows, ncols,
                  float(t), ctypes.addressof(prm), int(max_dist), It_out.data_ptr(), _ptr(Ut_out), _ptr(Vt_out), _ptr(source_out))
        return It_out, Ut_out, Vt_out, source_out
    old = capi.get_mode()
    if mode is not None:
        capi.set_mode(mode)
    try:
        capi.call("pdeip_flow_interpolate_dev", _stream(), *_p(I0, I1), channels, *_p(Uf, Vf), _ptr(Ub), _ptr(Vb), nrows, ncols, float(t),
                  ctypes.addressof(prm), It_out.data_ptr(), _ptr(Ut_out), _ptr(Vt_out), _ptr(source_out))
    finally:
        if mode is not None:
            capi.set_mode(old)
    return It_out, Ut_out, Vt_out, source_out


# ---- exact Euclidean distance transform, signed distance, nearest fill (csrc/pdeip_edt.hip) ----
EDT_MODES = {"positive": capi.EDT_POSITIVE, "nonneg": capi.EDT_NONNEG, "not_nan": capi.EDT_NOT_NAN, "positive_not": capi.EDT_POSITIVE_NOT,
             "nonneg_not": capi.EDT_NONNEG_NOT, "not_nan_not": capi.EDT_NOT_NAN_NOT}


def _typed_plane(like, given, wanted, dtype, what):
    if given is None and wanted:
        given = torch.empty(like.shape, dtype=dtype, device=like.device)
    if given is not None:
        _chk_typed(given, dtype, like.numel(), what)
    return given


def edt(A, mode="positive", max_dist=0, d2_out=None, idx_out=None, dist_out=None, d2=True, idx=True, dist=True):
    """The exact Euclidean distance transform of the resident plane A [(F,) ncols, nrows] (pdeip_edt_dev), every frame on its own.
    mode: which pixels are features -- 'positive' A > 0, 'nonneg' A >= 0, 'not_nan', each with a '_not' twin for the complement (or a
    PDEIP_EDT_* number).  Returns (d2, idx, dist): int32 squared distance, int32 0-based column-major index of the nearest feature
    within its frame (ties: the lowest index), float32 distance; INT32_MAX / -1 / +Inf where there is none (none at all, or none
    within max_dist > 0).  An output is None with d2 / idx / dist False unless handed in.  Nothing is read back."""
    _chk(A)
    if isinstance(mode, str) and mode not in EDT_MODES:
        raise capi.PdeipError(capi.PDEIP_ERR_ARG, "edt: unknown mode %r (one of %s)" % (mode, sorted(EDT_MODES)))
    nrows, ncols, F = _dims(A)
    d2_out = _typed_plane(A, d2_out, d2, torch.int32, "edt: d2_out")
    idx_out = _typed_plane(A, idx_out, idx, torch.int32, "edt: idx_out")
    dist_out = _typed_plane(A, dist_out, dist, torch.float32, "edt: dist_out")
    capi.call("pdeip_edt_dev", _stream(), A.data_ptr(), nrows, ncols, F, int(EDT_MODES.get(mode, mode)), int(max_dist), _ptr(d2_out),
              _ptr(idx_out), _ptr(dist_out))
    return d2_out, idx_out, dist_out


def bwdist(BW, D_out=None, idx_out=None, idx=True):
    """[D, IDX] = bwdist(BW > 0), Euclidean (pdeip_bwdist_dev): BW float32 [(F,) ncols, nrows].  Returns (D, IDX): float32 distance to
    the nearest positive pixel and its 0-based index (int32; -1 and +Inf in a frame without one; IDX None with idx=False unless handed
    in).  Nothing is read back."""
    _chk(BW)
    nrows, ncols, F = _dims(BW)
    D_out = _typed_plane(BW, D_out, True, torch.float32, "bwdist: D_out")
    idx_out = _typed_plane(BW, idx_out, idx, torch.int32, "bwdist: idx_out")
    capi.call("pdeip_bwdist_dev", _stream(), BW.data_ptr(), nrows, ncols, F, D_out.data_ptr(), _ptr(idx_out))
    return D_out, idx_out


def signed_distance(A, max_dist=0, out=None):
    """The signed Euclidean distance of the level set whose inside is A >= 0 (pdeip_signed_distance_dev): positive inside, negative
    outside, the interface half-way between an inside pixel and its outside neighbour (|out| >= 0.5).  max_dist = R > 0: values beyond
    the band saturate at +-(R + 0.5); otherwise a plane without an interface is +-Inf.  out may be A.  Returns out."""
    _chk(A)
    nrows, ncols, F = _dims(A)
    out = _typed_plane(A, out, True, torch.float32, "signed_distance: out")
    capi.call("pdeip_signed_distance_dev", _stream(), A.data_ptr(), nrows, ncols, F, int(max_dist), out.data_ptr())
    return out


def nearest_fill(D, max_dist=0, out=None, filled_out=None, dist_out=None):
    """The holes (NaN) of the resident sparse map D [(F,) ncols, nrows] take the bits of the nearest known pixel of their frame
    (pdeip_nearest_fill_dev; ties: the lowest index); known pixels keep their bits; a hole without a source (an empty frame, or none
    within max_dist > 0) stays NaN.  filled_out (optional) = 1 on the holes that were filled, dist_out (optional) = the distance to the
    source.  out may be D.  Returns out.  Not a substitute for tv_inpaint4 on occlusion bands: their nearest neighbour is the foreground."""
    _chk(D)
    nrows, ncols, F = _dims(D)
    out = _typed_plane(D, out, True, torch.float32, "nearest_fill: out")
    for t, what in ((filled_out, "filled_out"), (dist_out, "dist_out")):
        if t is not None:
            _chk_typed(t, torch.float32, D.numel(), "nearest_fill: " + what)
    capi.call("pdeip_nearest_fill_dev", _stream(), D.data_ptr(), nrows, ncols, F, int(max_dist), out.data_ptr(), _ptr(filled_out),
              _ptr(dist_out))
    return out


# ---- primal-dual total variation: TV-L1, ROF, Huber-TV (csrc/pdeip_tvpd.hip) ----
TVPD_MODELS = {"l1": capi.TVPD_L1, "l2": capi.TVPD_L2}


class TvpdParams(ctypes.Structure):
    """pdeip_tvpd_params: model PDEIP_TVPD_L1 / _L2, the data weight lambda, huber (0 = TV), iter, tau and sigma (NaN = 0.25 and 0.5)."""
    _fields_ = [("model", ctypes.c_int), ("lambda_", ctypes.c_double), ("huber", ctypes.c_double), ("iter", ctypes.c_int), ("tau", ctypes.c_double),
                ("sigma", ctypes.c_double)]

    @classmethod
    def make(cls, model, lam, iter, huber=0.0, tau=None, sigma=None, who="tv_pd"):
        if isinstance(model, str) and model.lower() not in TVPD_MODELS:
            raise ValueError("%s: model must be 'l1' or 'l2' (got %r)" % (who, model))
        nan = float("nan")
        return cls(int(TVPD_MODELS[model.lower()] if isinstance(model, str) else model), float(lam), float(huber), int(iter),
                   nan if tau is None else float(tau), nan if sigma is None else float(sigma))


def tv_pd(f, model, lam, iter, huber=0, u0=None, tau=None, sigma=None, out=None):
    """Primal-dual total variation of the resident plane f [(F,) ncols, nrows] (pdeip_tv_pd_dev), every frame on its own: `iter`
    iterations of Chambolle and Pock's method for TV + lam |u - f| (model 'l1', which rejects outliers) or TV + lam/2 (u - f)^2 ('l2',
    ROF), Huber-TV with huber > 0.  NaN in f means no data there.  The start is u0, or f with its holes filled from the nearest known
    pixel.  tau, sigma: None = 0.25 and 0.5.  f and u0 are not modified; out must be neither.  Returns out.  Nothing is read back."""
    _chk(f)
    prm = TvpdParams.make(model, lam, iter, huber, tau, sigma)
    nrows, ncols, F = _dims(f)
    if u0 is not None:
        _chk(u0)
        if u0.shape != f.shape:
            raise capi.PdeipError(capi.PDEIP_ERR_ARG, "tv_pd: u0 is %s but f is %s" % (tuple(u0.shape), tuple(f.shape)))
    out = _out_plane(f, out, True, "tv_pd: out")
    capi.call("pdeip_tv_pd_dev", _stream(), f.data_ptr(), _ptr(u0), nrows, ncols, F, ctypes.addressof(prm), out.data_ptr())
    return out


# ---- TV-L1 optical flow: the linearisation's rc and the primal-dual iteration (csrc/pdeip_tvl1.hip) ----
class Tvl1Params(ctypes.Structure):
    """pdeip_tvl1_params: the data weight lambda (NaN = 15), huber (0 = TV; NaN = 0), iter, tau and sigma (NaN = 0.25 and 0.5)."""
    _fields_ = [("lambda_", ctypes.c_double), ("huber", ctypes.c_double), ("iter", ctypes.c_int), ("tau", ctypes.c_double), ("sigma", ctypes.c_double)]

    @classmethod
    def make(cls, lam=None, iter=20, huber=None, tau=None, sigma=None):
        nan = float("nan")
        d = lambda v: nan if v is None else float(v)
        return cls(d(lam), d(huber), int(iter), d(tau), d(sigma))


class FlowTvl1Params(ctypes.Structure):
    """pdeip_flow_tvl1_params: a member that is <= 0 or NaN keeps the driver's default."""
    _fields_ = [("lambda_", ctypes.c_double), ("huber", ctypes.c_double), ("tau", ctypes.c_double), ("sigma", ctypes.c_double),
                ("scl_factor", ctypes.c_double), ("warps", ctypes.c_int), ("iter", ctypes.c_int), ("scales", ctypes.c_int)]


def tvl1_rc(I0, W, gx, gy, U0, V0, out=None):
    """rc = ((W - I0) - gx U0) - gy V0 of one warp's linearisation (pdeip_tvl1_rc_dev): planes [ncols, nrows]; NaN in W (the warp left
    the frame) makes rc NaN, "no data here".  Returns out."""
    _chk(I0, W, gx, gy, U0, V0)
    nrows, ncols, _ = _dims(U0)
    for t in (I0, W, gx, gy, V0):
        if t.numel() != U0.numel():
            raise capi.PdeipError(capi.PDEIP_ERR_ARG, "tvl1_rc: the planes must have one size")
    out = _out_plane(U0, out, True, "tvl1_rc: out")
    capi.call("pdeip_tvl1_rc_dev", _stream(), *_p(I0, W, gx, gy, U0, V0), nrows, ncols, out.data_ptr())
    return out


def tvl1_iterate(rc, gx, gy, U, V, lam=None, iter=20, huber=None, P=None, tau=None, sigma=None, out=None):
    """`iter` primal-dual iterations of TV-L1 flow on one linearisation (pdeip_tvl1_iterate_dev) from u = u_prev = U, v = v_prev = V.
    P [4, ncols, nrows]: the duals pxu, pyu, pxv, pyv, read and updated in place; None: zero duals, the result discarded.  lam, huber,
    tau, sigma: None = 15, 0, 0.25 and 0.5.  rc, gx, gy, U, V are not modified; out = (U_out, V_out) must be none of them.  Returns
    (U_out, V_out).  Nothing is read back."""
    _chk(rc, gx, gy, U, V)
    nrows, ncols, _ = _dims(U)
    for t in (rc, gx, gy, V):
        if t.numel() != U.numel():
            raise capi.PdeipError(capi.PDEIP_ERR_ARG, "tvl1_iterate: the planes must have one size")
    if P is not None:
        _chk(P)
        if P.numel() != 4 * U.numel():
            raise capi.PdeipError(capi.PDEIP_ERR_ARG, "tvl1_iterate: P is %s, not four planes of %s" % (tuple(P.shape), tuple(U.shape)))
    Uo, Vo = (None, None) if out is None else out
    Uo, Vo = _out_plane(U, Uo, True, "tvl1_iterate: U_out"), _out_plane(V, Vo, True, "tvl1_iterate: V_out")
    prm = Tvl1Params.make(lam, iter, huber, tau, sigma)
    capi.call("pdeip_tvl1_iterate_dev", _stream(), *_p(rc, gx, gy, U, V), _ptr(P), nrows, ncols, ctypes.addressof(prm), *_p(Uo, Vo))
    return Uo, Vo
