"""numpy restatement of matlab/diffusion/Diffusion4_v10.m, the nonlinear (lagged-diffusivity) diffusion filter: the checker of
csrc/pdeip_diffusion.hpp / pdeip_diffusion4.

Independent of the product (nothing in the package imports this file).  Every line of a solve is handled at once, vectorised
across lines, with the recurrence stepping along the line axis.  Arrays use MATLAB's shape convention [rows, cols] or
[rows, cols, C].  `dtype` is the precision every operation is rounded to: float32 is the contract (MATLAB's single, each
operation rounded in the order the .m states it; numpy forms no FMA), float64 is only for checking the algebra.  A double
scalar meets a single array rounded to single.

  DiffWeights   :97-127   weights of the channel maximum: 1./realsqrt(w + 0.00001), outer column / row zeroed
  TDMA          :70-92    Thomas solve along axis 0
  the loop      :41-62    Iout = single(I_in); for iter = 0:outer_iter, Iout(:,:,k) = ver + hor
  uint8(Iout)   :64       round half away from zero, saturate to 0..255, NaN -> 0
"""
import math

import numpy as np


def _shift(A, di, dj):
    """circshift(A, [di dj 0]): element (i, j) takes A(i - di, j - dj), wrapping."""
    return np.roll(np.roll(A, di, axis=0), dj, axis=1)


def diff_weights(D, dtype=np.float32, channel_max=None, eps=0.00001):
    """[wW wN wE wS] = DiffWeights(D) (:97-127) as [rows, cols] planes.  `channel_max` (the .m's max(w, [], 3) = np.fmax.reduce when
    None) and `eps` (the .m's 0.00001) are open only so that tests/diffusion_nan_cases.py can state the C gateway's rule next to the
    .m's with the same arithmetic around it."""
    channel_max = channel_max or (lambda T: np.fmax.reduce(T, axis=2))  # max(w, [], 3): NaN omitted, as MATLAB's max
    t = np.dtype(dtype).type
    D = np.asarray(D, dtype)
    if D.ndim == 2:
        D = D[:, :, None]
    with np.errstate(all="ignore"):
        P = np.pad(D, ((1, 1), (0, 0), (0, 0)), mode="edge")
        Dver = t(0.25) * P[:-2] - t(0.25) * P[2:]  # imfilter(D, [0.25 0 -0.25]', 'replicate')
        P = np.pad(D, ((0, 0), (1, 1), (0, 0)), mode="edge")
        Dhor = t(0.25) * P[:, :-2] - t(0.25) * P[:, 2:]  # imfilter(D, [0.25 0 -0.25], 'replicate')

        def w(di, dj, Dd):
            A = _shift(D, di, dj) - D
            B = Dd + _shift(Dd, di, dj)
            m = channel_max(A * A + B * B)
            return (t(1) / np.sqrt(m + t(eps))).astype(dtype)

        wW, wE = w(0, 1, Dver), w(0, -1, Dver)
        wN, wS = w(1, 0, Dhor), w(-1, 0, Dhor)
    wW[:, 0] = 0
    wE[:, -1] = 0
    wN[0, :] = 0
    wS[-1, :] = 0
    return wW, wN, wE, wS


def tdma(a, b, c, d):
    """x = TDMA(a, b, c, d) (:70-92): every column of the [n, m] arrays is one system, solved in their dtype."""
    a, b, c, d = (np.array(v) for v in (a, b, c, d))
    n = a.shape[0]
    if n < 2:
        raise ValueError("TDMA needs lines of at least 2 elements (MATLAB indexes d(0) below that)")
    one = a.dtype.type(1)
    with np.errstate(all="ignore"):
        c[0] = c[0] / b[0]
        d[0] = d[0] / b[0]
        for i in range(1, n - 1):
            temp = one / (b[i] - a[i] * c[i - 1])
            c[i] = c[i] * temp
            d[i] = (d[i] - a[i] * d[i - 1]) * temp
        d[n - 1] = (d[n - 1] - a[n - 1] * d[n - 2]) / (b[n - 1] - a[n - 1] * c[n - 2])
        x = np.empty_like(d)
        x[n - 1] = d[n - 1]
        for i in range(n - 2, -1, -1):
            x[i] = d[i] - c[i] * x[i + 1]
    return x


def outer_iteration(I, alpha, dtype=np.float32, channel_max=None):
    """One pass of the loop body (:46-61) on I [rows, cols, C]; returns the new Iout."""
    t = np.dtype(dtype).type
    I = np.asarray(I, dtype)
    al = t(alpha)
    wW, wN, wE, wS = diff_weights(I, dtype, channel_max)
    with np.errstate(all="ignore"):
        a_ver, b_ver, c_ver = (-al) * wN, t(2) + al * (wN + wS), (-al) * wS
        a_hor, b_hor, c_hor = ((-al) * wW).T, (t(2) + al * (wW + wE)).T, ((-al) * wE).T
        out = np.empty_like(I)
        for k in range(I.shape[2]):
            ver = tdma(a_ver, b_ver, c_ver, I[:, :, k])
            hor = tdma(a_hor, b_hor, c_hor, I[:, :, k].T).T
            out[:, :, k] = ver + hor
    return out


def iterations(outer_iter):
    """Iterations of `for iter = 0:outer_iter`."""
    return int(math.floor(outer_iter)) + 1 if outer_iter >= 0 else 0


def Diffusion4_v10(I_in, alpha=25, outer_iter=5, dtype=np.float32, channel_max=None):
    """Iout of Diffusion4_v10(I_in, 'alpha', alpha, 'outer_iter', outer_iter) before uint8 (:41-62), in I_in's shape."""
    I = np.asarray(I_in, dtype=np.float32).astype(dtype)
    shape = I.shape
    if I.ndim == 2:
        I = I[:, :, None]
    for _ in range(iterations(outer_iter)):
        I = outer_iteration(I, alpha, dtype, channel_max)
    return np.asfortranarray(I.reshape(shape))


def to_uint8(x):
    """uint8(x) (:64): round half away from zero, saturate to 0..255, NaN -> 0."""
    x = np.asarray(x, dtype=np.float64)
    r = np.where(x >= 0, np.floor(np.abs(x) + 0.5), -np.floor(np.abs(x) + 0.5))
    r = np.where(np.isnan(x), 0.0, r)
    return np.clip(r, 0, 255).astype(np.uint8)
