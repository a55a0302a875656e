"""The NumPy restatement of the frame interpolation of include/pdeip.h (pdeip_flow_splat_dev, pdeip_interp_blend_dev,
pdeip_flow_interpolate): float64 on the promoted float32 inputs, every product and sum a separate rounded operation in the order the
header gives.  The sampler is crosscheck_ref.sample_xy, the hole filling inpaint_ref.tv_inpaint4, the masks
crosscheck_ref.flow_crosscheck.  Pinned by test_interp_ref.py; tests/test_gpu_interp.py compares the GPU with it bit for bit.
Arrays are MATLAB-shaped [nrows, ncols(, C)]."""
import numpy as np

import crosscheck_ref as cr
import inpaint_ref as ir

F32, F64 = np.float32, np.float64
EMPTY = (1 << 64) - 1


def _c3(A):
    A = np.asarray(A, dtype=F32)
    return A if A.ndim == 3 else A[:, :, None]


def _grid(nrows, ncols):
    return np.arange(1, ncols + 1, dtype=F64)[None, :], np.arange(1, nrows + 1, dtype=F64)[:, None]


def splat_costs(Uf, Vf, I0=None, I1=None):
    """c of every pixel as float32 (meaningful on sources only): 0 without images."""
    Uf, Vf = np.asarray(Uf, F32), np.asarray(Vf, F32)
    nrows, ncols = Uf.shape
    if I0 is None:
        return np.zeros((nrows, ncols), F32)
    A0, A1 = _c3(I0), _c3(I1)
    x, y = _grid(nrows, ncols)
    with np.errstate(invalid="ignore", over="ignore"):
        xq, yq = x + Uf.astype(F64), y + Vf.astype(F64)
        total = np.zeros((nrows, ncols), F64)
        for ch in range(A0.shape[2]):
            total = total + np.abs(A0[:, :, ch].astype(F64) - cr.sample_xy(A1[:, :, ch], xq, yq))
        c = total.astype(F32)
    return np.where(np.isnan(c), F32(np.inf), c).astype(F32)   # out of range is a NaN sample, hence a NaN sum


def flow_splat(Uf, Vf, t, I0=None, I1=None):
    """-> Ut, Vt, cost (float32 planes, NaN on holes), winner (int64 plane: the winning source's linear index, -1 on holes)."""
    Uf, Vf = np.asfortranarray(np.asarray(Uf, F32)), np.asfortranarray(np.asarray(Vf, F32))
    nrows, ncols = Uf.shape
    t = float(t)
    cost = splat_costs(Uf, Vf, I0, I1)
    bits = cost.view(np.uint32)
    keys = [EMPTY] * (nrows * ncols)          # by linear index j * nrows + i
    source = np.isfinite(Uf) & np.isfinite(Vf)
    for j in range(ncols):
        for i in range(nrows):
            if not source[i, j]:
                continue
            p = j * nrows + i
            key = (int(bits[i, j]) << 32) | p
            xq = float(j + 1) + t * float(Uf[i, j])
            yq = float(i + 1) + t * float(Vf[i, j])
            fx, fy = np.floor(xq), np.floor(yq)
            cols = [fx] + ([fx + 1.0] if xq != fx else [])
            rows = [fy] + ([fy + 1.0] if yq != fy else [])
            for c in cols:
                if not 1.0 <= c <= float(ncols):
                    continue
                for r in rows:
                    if not 1.0 <= r <= float(nrows):
                        continue
                    q = (int(c) - 1) * nrows + (int(r) - 1)
                    if key < keys[q]:
                        keys[q] = key
    Ut, Vt, ct = (np.full((nrows, ncols), np.nan, F32, order="F") for _ in range(3))
    winner = np.full((nrows, ncols), -1, np.int64, order="F")
    uf, vf = Uf.reshape(-1, order="F"), Vf.reshape(-1, order="F")
    for q, key in enumerate(keys):
        if key == EMPTY:
            continue
        p = key & 0xffffffff
        i, j = q % nrows, q // nrows
        Ut[i, j], Vt[i, j] = uf[p], vf[p]
        ct[i, j] = np.array([key >> 32], np.uint32).view(F32)[0]
        winner[i, j] = p
    return Ut, Vt, ct, winner


def _nearest(M, xq, yq, ok):
    """M at column min(floor(xq + 0.5), ncols), row alike (1-based), != 0; True without a mask.  Evaluated where ok."""
    if M is None:
        return np.ones(xq.shape, bool)
    nrows, ncols = M.shape
    xs, ys = np.where(ok, xq, 1.0), np.where(ok, yq, 1.0)
    c = np.minimum(np.floor(xs + 0.5), float(ncols)).astype(np.int64) - 1
    r = np.minimum(np.floor(ys + 0.5), float(nrows)).astype(np.int64) - 1
    return np.asarray(M, F32)[r, c] != 0


def interp_blend(I0, I1, Ut, Vt, t, M0=None, M1=None):
    """-> It (float32, the shape of I0), source (float32 plane)."""
    A0, A1 = _c3(I0), _c3(I1)
    Ut, Vt = np.asarray(Ut, F32), np.asarray(Vt, F32)
    nrows, ncols = Ut.shape
    t = float(t)
    tq = 1.0 - t
    x, y = _grid(nrows, ncols)
    fin = np.isfinite(Ut) & np.isfinite(Vt)
    with np.errstate(invalid="ignore", over="ignore"):
        u, v = Ut.astype(F64), Vt.astype(F64)
        x0, y0 = x - t * u, y - t * v
        x1, y1 = x + tq * u, y + tq * v
        in0 = (x0 >= 1.0) & (x0 <= float(ncols)) & (y0 >= 1.0) & (y0 <= float(nrows))
        in1 = (x1 >= 1.0) & (x1 <= float(ncols)) & (y1 >= 1.0) & (y1 <= float(nrows))
    r0, r1 = fin & in0, fin & in1
    p0, p1 = _nearest(M0, x0, y0, r0), _nearest(M1, x1, y1, r1)
    both = r0 & r1
    src = np.where(both, np.where(p0 == p1, 3, np.where(p0, 2, 1)), np.where(r0, 1, np.where(r1, 2, 0)))
    It = np.empty(A0.shape, F32, order="F")
    for ch in range(A0.shape[2]):
        with np.errstate(invalid="ignore", over="ignore"):
            a0 = cr.sample_xy(A0[:, :, ch], np.where(r0, x0, np.nan), np.where(r0, y0, np.nan))
            a1 = cr.sample_xy(A1[:, :, ch], np.where(r1, x1, np.nan), np.where(r1, y1, np.nan))
            mix = (tq * a0 + t * a1).astype(F32)
            It[:, :, ch] = np.where(src == 3, mix, np.where(src == 1, a0.astype(F32), np.where(src == 2, a1.astype(F32), F32(np.nan))))
    return np.asfortranarray(It.reshape(np.shape(I0))), np.asfortranarray(src.astype(F32))


def flow_interpolate(orc, I0, I1, Uf, Vf, Ub=None, Vb=None, t=0.5, a=0.01, b=0.5, use_costs=1, **fill):
    """-> It, Ut, Vt (the filled flow at t), source.  fill: inpaint_ref.tv_inpaint4's parameters (order: the oracle's sweep order)."""
    M0 = M1 = None
    if Ub is not None:
        M0 = cr.flow_crosscheck(Uf, Vf, Ub, Vb, a, b)["mask"]
        M1 = cr.flow_crosscheck(Ub, Vb, Uf, Vf, a, b)["mask"]
    Ut, Vt, _, _ = flow_splat(Uf, Vf, t, I0 if use_costs else None, I1 if use_costs else None)
    filled, _ = ir.tv_inpaint4(orc, np.asfortranarray(np.stack([Ut, Vt], axis=2)), **fill)
    Ut, Vt = np.asfortranarray(filled[:, :, 0]), np.asfortranarray(filled[:, :, 1])
    It, src = interp_blend(I0, I1, Ut, Vt, t, M0, M1)
    return It, Ut, Vt, src
