"""numpy float32 restatement of the reference's Chan-Vese AOS step (CV_solver_2d) and of the terms its drivers build for it:
the checker of csrc/pdeip_cv.hpp.

Independent of the product (nothing in the package imports this file).  Every line of a pass is solved at once, vectorised
across lines, with the recurrence stepping along the line axis; the line helpers (_lines, _coefficients, _thomas_forward) are
levelset_ref's.  Arrays use MATLAB's shape convention [nrows, ncols] or [nrows, ncols, nframes], float32 throughout with the
reference's association (numpy forms no FMA).

Reference (mex/source/library/levelsetSolvers.c, GRADNORM_ZERO_CHECK defined, PMIN/PMAX = -5/+5):
  CV_solver_2d.c     gateway: PHI_out = CV_solver_2d(PHI, D, DH, GradNorm, tau, nu) -> CV_AOSOMP_4_2d (:103)
  CV_TDMA_Column4_omp  :189   column pass into a zero-filled output
  CV_TDMA_Row4_omp     :305   row pass adding to the column result
The gateway hands DH to the library's GradNorm_in slot and GradNorm to its Diff_in slot, so with g = GradNorm, delta = DH:
  w(p, q) = (g_p + g_q > 0) ? ((2*tau)*delta_p) / (g_p + g_q) : 0,      d_p = PHI_p + (tau*delta_p)*D_p
and the back-substitution chain always runs on the solved x: the column and row solves are independent, and
  col = (i >= 1 && g == 0) ? clamp(PHI) : clamp(0 + xc),   out = (j >= 1 && g == 0) ? clamp(PHI) : clamp(col + xr).
"""
import numpy as np

import levelset_ref as ls

F32 = np.float32
PMIN, PMAX = F32(-5), F32(5)


def clamp(v):
    """if (v > PMAX) v = PMAX; if (v < PMIN) v = PMIN; -- a NaN passes through."""
    v = np.where(v > PMAX, PMAX, v)
    return np.where(v < PMIN, PMIN, v).astype(F32)


def line_solve(PHI, D, DH, GradNorm, tau, nu, axis):
    """x of the Thomas solve along every column (axis 0) or row (axis 1), before any output rule."""
    tau, nu = F32(tau), F32(nu)
    shape = ls._f(PHI).shape
    P, Dd, H, G = (ls._lines(x, axis) for x in (PHI, D, DH, GradNorm))
    a, b, c, _ = ls._coefficients(P, Dd, H, G, tau, nu)  # harm() with Diff := GradNorm, GN := DH
    d = (P + (tau * H) * Dd).astype(F32)
    cp, dp = ls._thomas_forward(a, b, c, d)
    n = P.shape[0]
    X = np.empty_like(P)
    X[n - 1] = dp[n - 1]
    with np.errstate(all="ignore"):
        for k in range(n - 2, -1, -1):
            X[k] = dp[k] - cp[k] * X[k + 1]
    return ls._unlines(X, shape, axis)


def CV_solver_2d(PHI, D, DH, GradNorm, tau, nu):
    """PHI_out = CV_solver_2d(PHI, D, DH, GradNorm, tau, nu) (CV_AOSOMP_4_2d)."""
    P, G = ls._f(PHI), ls._f(GradNorm)
    xc = line_solve(PHI, D, DH, GradNorm, tau, nu, 0)
    xr = line_solve(PHI, D, DH, GradNorm, tau, nu, 1)
    zero = G == F32(0)
    i = np.arange(P.shape[0])[:, None]
    j = np.arange(P.shape[1])[None, :]
    if P.ndim == 3:
        i, j = i[..., None], j[..., None]
    with np.errstate(all="ignore"):
        col = np.where((i >= 1) & zero, clamp(P), clamp(F32(0) + xc))
        out = np.where((j >= 1) & zero, clamp(P), clamp(col + xr))
    return np.asfortranarray(out.astype(F32))


def cv_terms(PHI, c0, c1, dh_floor=np.nan):
    """DH and gradPHI of the segmentation drivers (DispSegmentation.m:380-387, DispSegmentationSparse.m:388-396), this
    library's definition for single PHI: DH = 1/(pi*(c0 + PHI^2/c1)), floored where a floor is given (NaN: none; a NaN DH
    stays NaN); gradPHI = sqrt(dx^2 + dy^2) with imfilter(PHI, [-1 0 1]*0.5, 'replicate') and its transpose."""
    P = ls._f(PHI)
    c0, c1, fl = F32(c0), F32(c1), F32(dh_floor)
    with np.errstate(all="ignore"):
        DH = F32(1) / (F32(np.pi) * (c0 + (P * P) / c1))
        DH = np.where(DH < fl, fl, DH).astype(F32)
        dx, dy = ls._imfilter3(P, 1, ls._DX), ls._imfilter3(P, 0, ls._DX)
        G = np.sqrt(dx * dx + dy * dy).astype(F32)
    return np.asfortranarray(DH), np.asfortranarray(G)
