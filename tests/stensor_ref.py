"""numpy restatement of structure-tensor anisotropic diffusion (Weickert's EED and CED) as include/pdeip.h states it: the checker of
csrc/pdeip_stensor.hpp / pdeip_gauss, pdeip_structure_tensor_dev, pdeip_st_weights_dev, pdeip_diffusion8.

Independent of the product (nothing in the package imports this file).  Arrays use MATLAB's shape convention [rows, cols] or
[rows, cols, C]; x runs along the columns (axis 1), y down the rows (axis 0).  The Gaussian and the tensor products are float32
with every operation rounded in the stated order (numpy forms no FMA); the diffusion tensor and the weights are float64 from the
float32 J, rounded to float32 at the end.  One step's solve is oracle_lib.PDEsolver8, the reference's own solver.
"""
import math
from fractions import Fraction

import numpy as np

F32 = np.float32
RMAX = 32
DEFAULTS = {"ced": dict(sigma=0.7, rho=4.0, alpha=0.001, C=1.0, **{"lambda": 6.0}),
            "eed": dict(sigma=1.5, rho=0.0, alpha=0.001, C=1.0, **{"lambda": 6.0})}
COMMON = dict(tau=1.0, iters=10, inner_iter=4, omega=1.0, solver=1)


def params(mode="ced", **param):
    p = dict(DEFAULTS[mode], **COMMON)
    for k, v in param.items():
        if k not in p:
            raise TypeError("unknown parameter %r" % k)
        p[k] = v
    return p


# ---- Gaussian ---------------------------------------------------------------------------------------------------------------

def radius(sigma):
    """ceil(3 sigma) of the exact product (the double product may round down onto an integer that the exact one exceeds)."""
    return int(math.ceil(3 * Fraction(sigma)))


def taps(sigma):
    """g[k] = exp(-k^2 / (2 sigma^2)), k = -R..R, in double, over their double sum (ascending k), each rounded to float32.  A sigma
    whose square underflows to zero divides by it as IEEE does: exp(-inf) = 0, the centre tap alone."""
    R = radius(sigma)
    if R > RMAX:
        raise ValueError("sigma = %g needs a radius above %d" % (sigma, RMAX))
    den = 2.0 * sigma * sigma
    g = [1.0 if k == 0 else (math.exp(-float(k * k) / den) if den > 0.0 else 0.0) for k in range(-R, R + 1)]
    s = 0.0
    for v in g:
        s += v
    return np.array([v / s for v in g], dtype=np.float64).astype(F32)


def smooth_axis(A, g, axis):
    """((g[0] x[-R] + g[1] x[-R+1]) + ...) + g[2R] x[R] along `axis`, replicate border, float32 tap by tap."""
    g = np.asarray(g, F32)
    R = (len(g) - 1) // 2
    A = np.asarray(A, F32)
    pad = [(0, 0)] * A.ndim
    pad[axis] = (R, R)
    P = np.pad(A, pad, mode="edge")
    n = A.shape[axis]
    with np.errstate(all="ignore"):
        acc = None
        for k in range(2 * R + 1):
            term = g[k] * np.take(P, np.arange(k, k + n), axis=axis)
            acc = term if acc is None else acc + term
    assert acc.dtype == F32
    return acc


def gaussian(A, sigma, g=None):
    """G_sigma * A: along the rows (axis 0) first, rounded to float32, then along the columns (axis 1).  `g`: taps to use instead of
    taps(sigma) (the GPU tests hand over the library's own)."""
    g = taps(sigma) if g is None else np.asarray(g, F32)
    A = np.asarray(A, F32)
    if len(g) == 1:
        return A.copy()
    return smooth_axis(smooth_axis(A, g, 0), g, 1)


def gaussian_direct64(A, sigma):
    """The same filter as one 2-D convolution in float64 with the float64 taps (for checking the separable form)."""
    R = radius(sigma)
    g = np.array([math.exp(-float(k * k) / (2.0 * sigma * sigma)) if k else 1.0 for k in range(-R, R + 1)])
    g = g / g.sum()
    A = np.asarray(A, np.float64)
    P = np.pad(A, ((R, R), (R, R)) + ((0, 0),) * (A.ndim - 2), mode="edge")
    out = np.zeros_like(A)
    for a in range(2 * R + 1):
        for b in range(2 * R + 1):
            out += g[a] * g[b] * P[a:a + A.shape[0], b:b + A.shape[1]]
    return out


# ---- structure tensor -------------------------------------------------------------------------------------------------------

_S = 4.0 + math.sqrt(8.0)
W1, W2 = F32(1.0 / _S), F32(math.sqrt(2.0) / _S)


def derivatives(V):
    """gx (toward increasing column), gy (toward increasing row) of one plane: Alvarez 3x3, replicate border, float32."""
    P = np.pad(np.asarray(V, F32), 1, mode="edge")
    with np.errstate(all="ignore"):
        dx = P[:, 2:] - P[:, :-2]   # [rows + 2, cols]: v(., j+1) - v(., j-1) on every padded row
        gx = (W1 * dx[:-2] + W2 * dx[1:-1]) + W1 * dx[2:]
        dy = P[2:, :] - P[:-2, :]   # [rows, cols + 2]
        gy = (W1 * dy[:, :-2] + W2 * dy[:, 1:-1]) + W1 * dy[:, 2:]
    return gx, gy


def products(V):
    """J11, J12, J22 = sum_c gx^2, gx gy, gy^2, float32, channel 0's product first, the others added in index order."""
    V = np.asarray(V, F32)
    V = V[:, :, None] if V.ndim == 2 else V
    J = None
    with np.errstate(all="ignore"):
        for c in range(V.shape[2]):
            gx, gy = derivatives(V[:, :, c])
            p = [gx * gx, gx * gy, gy * gy]
            J = p if J is None else [a + b for a, b in zip(J, p)]
    return np.stack(J, axis=2)


def structure_tensor(I, sigma, rho, gs=None, gr=None):
    """J [rows, cols, 3] = G_rho * products(G_sigma * I)."""
    I = np.asarray(I, F32)
    I = I[:, :, None] if I.ndim == 2 else I
    return gaussian(products(gaussian(I, sigma, gs)), rho, gr)


# ---- diffusion tensor and weights --------------------------------------------------------------------------------------------

def diffusion_tensor(J, mode, p):
    """D11, D22, D12 in float64 from the float32 J [rows, cols, 3]."""
    j11, j12, j22 = (np.asarray(J[:, :, k], F32).astype(np.float64) for k in range(3))
    with np.errstate(all="ignore"):
        s, d = j11 + j22, j11 - j22
        r = np.sqrt(d * d + 4.0 * j12 * j12)
        mu1 = 0.5 * (s + r)
        pos = r > 0.0
        rs = np.where(pos, r, 1.0)
        c2 = np.where(pos, d / rs, 1.0)
        s2 = np.where(pos, 2.0 * j12 / rs, 0.0)
        if mode == "ced":
            a, C = float(p["alpha"]), float(p["C"])
            l1 = np.full_like(r, a)
            l2 = np.where(pos, a + (1.0 - a) * np.exp(-C / (rs * rs)), a)
        else:
            lam = float(p["lambda"])
            q = mu1 / (lam * lam)
            q2 = q * q
            l1 = np.where(mu1 > 0.0, 1.0 - np.exp(-3.31488 / (q2 * q2)), 1.0)
            l2 = np.ones_like(r)
        m, h = 0.5 * (l1 + l2), 0.5 * (l1 - l2)
        return m + h * c2, m - h * c2, h * s2


def exp_terms(J, mode, p):
    """(taken, value): where diffusion_tensor() takes an exp (CED: r > 0, EED: mu1 > 0) and what numpy's exp returns there, from the
    same float64 operations in the same order; `value` is NaN where none is taken."""
    j11, j12, j22 = (np.asarray(J[:, :, k], F32).astype(np.float64) for k in range(3))
    with np.errstate(all="ignore"):
        s, d = j11 + j22, j11 - j22
        r = np.sqrt(d * d + 4.0 * j12 * j12)
        mu1 = 0.5 * (s + r)
        if mode == "ced":
            taken = r > 0.0
            rs = np.where(taken, r, 1.0)
            value = np.exp(-float(p["C"]) / (rs * rs))
        else:
            taken = mu1 > 0.0
            lam = float(p["lambda"])
            q = np.where(taken, mu1, 1.0) / (lam * lam)
            q2 = q * q
            value = np.exp(-3.31488 / (q2 * q2))
    return taken, np.where(taken, value, np.nan)


def _shift(A, di, dj):
    """circshift(A, [di dj]): element (i, j) takes A(i - di, j - dj), wrapping."""
    return np.roll(np.roll(A, di, axis=0), dj, axis=1)


def weights64(D11, D22, D12):
    """The eight weights W NW N NE E SE S SW of TVdenoise8's assembly with dyy := D11, dxx := D22, dxy := D12, float64, the weights
    across the frame's edge zeroed; and their sum, left to right."""
    dyy, dxx, dxy = D11, D22, D12
    with np.errstate(all="ignore"):
        w = [0.5 * (dyy + _shift(dyy, 0, 1)), 0.25 * (dxy + _shift(dxy, 1, 1)), 0.5 * (dxx + _shift(dxx, 1, 0)),
             -0.25 * (dxy + _shift(dxy, 1, -1)), 0.5 * (dyy + _shift(dyy, 0, -1)), 0.25 * (dxy + _shift(dxy, -1, -1)),
             0.5 * (dxx + _shift(dxx, -1, 0)), -0.25 * (dxy + _shift(dxy, -1, 1))]
    for k in (0, 1, 7):
        w[k][:, 0] = 0.0    # W, NW, SW: first column
    for k in (3, 4, 5):
        w[k][:, -1] = 0.0   # NE, E, SE: last column
    for k in (1, 2, 3):
        w[k][0, :] = 0.0    # NW, N, NE: first row
    for k in (5, 6, 7):
        w[k][-1, :] = 0.0   # SE, S, SW: last row
    with np.errstate(all="ignore"):
        total = w[0] + w[1]
        for k in range(2, 8):
            total = total + w[k]
    return w, total


def st_weights(J, mode, p, tau):
    """TRACE = float32(1 + tau sum w), w8 = [float32(tau w_k)] in the order W NW N NE E SE S SW."""
    w, total = weights64(*diffusion_tensor(J, mode, p))
    tau = float(tau)
    with np.errstate(all="ignore"):
        return (1.0 + tau * total).astype(F32), [(tau * v).astype(F32) for v in w]


def apply_stencil(u, w):
    """sum_k w_k (u_k - u) in float64 for weights in the order W NW N NE E SE S SW (wrap-around neighbours: the frame weights are zero)."""
    nb = [_shift(u, 0, 1), _shift(u, 1, 1), _shift(u, 1, 0), _shift(u, 1, -1), _shift(u, 0, -1), _shift(u, -1, -1), _shift(u, -1, 0),
          _shift(u, -1, 1)]
    return sum(wk * (uk - u) for wk, uk in zip(w, nb))


# ---- one step and the driver ------------------------------------------------------------------------------------------------

def pad_weights(TRACE, w8):
    """TRACE and the weights on planes with a one-pixel ring: TRACE = 1 and zero weights there."""
    return (np.asfortranarray(np.pad(TRACE, 1, constant_values=F32(1))), [np.asfortranarray(np.pad(w, 1, constant_values=F32(0))) for w in w8])


def pad_image(X):
    """A plane inside a one-pixel ring of its nearest pixels."""
    return np.asfortranarray(np.pad(np.asarray(X, F32), 1, mode="edge"))


def step_padded(Xp, TRACEp, w8p, p, order=0):
    """PDEsolver8 on one ringed plane with B = the plane: the reference's solver relaxes the interior, which is the whole image."""
    import oracle_lib

    return oracle_lib.PDEsolver8(Xp, TRACEp, Xp, *w8p, int(p["inner_iter"]), float(p["omega"]), solver=int(p["solver"]), order=order)


def step(I, TRACE, w8, p, order=0):
    """One semi-implicit step of every channel with given weights [rows, cols]: pad, PDEsolver8 with B = X, crop.  PDEsolver8 never
    relaxes a plane's outer ring (it copies the neighbours there after every sweep), so the image is solved inside a ring of its
    own: every image pixel is relaxed, with zero weights across the image's edge."""
    I = np.asarray(I, F32)
    I3 = I[:, :, None] if I.ndim == 2 else I
    Tp, wp = pad_weights(TRACE, w8)
    out = np.empty(I3.shape, F32, order="F")
    for c in range(I3.shape[2]):
        out[:, :, c] = step_padded(pad_image(I3[:, :, c]), Tp, wp, p, order)[1:-1, 1:-1]
    return out if I.ndim == 3 else out[:, :, 0]


def Diffusion8(I_in, mode="ced", order=0, **param):
    """The whole filter in float32: Iout = single(I_in), then `iters` times J, weights, one step."""
    p = params(mode, **param)
    I = np.asfortranarray(np.asarray(I_in, F32))
    for _ in range(max(int(math.floor(p["iters"])), 0)):
        J = structure_tensor(I, p["sigma"], p["rho"])
        TRACE, w8 = st_weights(J, mode, p, p["tau"])
        I = step(I, TRACE, w8, p, order)
    return I


# ---- the quality scene of DESIGN 5.18 ------------------------------------------------------------------------------------------

def stripe_scene():
    """96 x 128 bent stripes and the same plus N(0, 40) noise: (clean, noisy), float64."""
    y, x = np.meshgrid(np.arange(96.0), np.arange(128.0), indexing="ij")
    clean = 128.0 + 90.0 * np.sin(0.55 * (x * math.cos(0.6) + y * math.sin(0.6)) + 1.5 * np.sin(y / 25.0))
    return clean, clean + np.random.default_rng(7).normal(0.0, 40.0, clean.shape)


def rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))
