"""The NumPy restatement of the cross-checks of include/pdeip.h (pdeip_disp_crosscheck, pdeip_flow_crosscheck): float64 on the
promoted float32 inputs, every product and sum a separate rounded operation in the order the header gives.  Pinned independently by
test_crosscheck_ref.py; tests/test_gpu_crosscheck.py compares the GPU with it bit for bit."""
import math

import numpy as np

F32, F64 = np.float32, np.float64


def warp_x(D1, D0):
    """w of the disparity check: D1 sampled linearly along x at xq = (j+1) + D0, NaN outside 1 <= xq <= ncols, xq == ncols the last
    column itself.  A tap with weight 0 still propagates its NaN."""
    nrows, ncols = D0.shape
    A = D1.astype(F64)
    xq = np.arange(1, ncols + 1, dtype=F64)[None, :] + D0.astype(F64)
    with np.errstate(invalid="ignore"):
        ok = (xq >= 1.0) & (xq <= float(ncols))
    xs = np.where(ok, xq, 1.0)
    j0 = np.minimum(np.floor(xs), float(ncols - 1))
    s = xs - j0
    c0 = j0.astype(np.int64) - 1
    c1 = np.minimum(c0 + 1, ncols - 1)
    ii = np.arange(nrows)[:, None]
    with np.errstate(invalid="ignore"):
        out = A[ii, c0] * (1.0 - s) + A[ii, c1] * s
    return np.where(ok, out, np.nan)


def _stats(kept, defined, mag):
    n = int(defined.sum())
    vals = mag[defined]
    return dict(kept=int(kept.sum()), defined=n, mean=(math.fsum(vals.tolist()) / n if n else math.nan),
                max=(float(vals.max()) if n else math.nan))


def disp_crosscheck(D0, D1, tol):
    """-> dict: sparse, mask, diff (float32 planes), r (float64), kept_mask, defined_mask, kept, defined, mean (math.fsum), max."""
    D0 = np.asarray(D0, F32)
    D1 = np.asarray(D1, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        r = D0.astype(F64) + warp_x(D1, D0)
        mag = np.abs(r)
        defined = np.isfinite(r)
        kept = defined & (mag <= tol)
        diff = r.astype(F32)
    sparse = np.where(kept, D0, F32(np.nan)).astype(F32)
    out = dict(sparse=sparse, mask=kept.astype(F32), diff=diff, r=r, kept_mask=kept, defined_mask=defined)
    out.update(_stats(kept, defined, mag))
    return out


def sample_xy(A, xq, yq):
    """B(A) of the flow check at the 1-based queries (xq along columns, yq along rows), NaN out of range."""
    nrows, ncols = A.shape
    A = A.astype(F64)
    with np.errstate(invalid="ignore"):
        ok = (xq >= 1.0) & (xq <= float(ncols)) & (yq >= 1.0) & (yq <= float(nrows))
    xs, ys = np.where(ok, xq, 1.0), np.where(ok, yq, 1.0)
    j0 = np.minimum(np.floor(xs), float(ncols - 1))
    i0 = np.minimum(np.floor(ys), float(nrows - 1))
    s, t = xs - j0, ys - i0
    c0 = j0.astype(np.int64) - 1
    r0 = i0.astype(np.int64) - 1
    c1, r1 = np.minimum(c0 + 1, ncols - 1), np.minimum(r0 + 1, nrows - 1)
    with np.errstate(invalid="ignore"):
        top = A[r0, c0] * (1.0 - s) + A[r0, c1] * s
        bot = A[r1, c0] * (1.0 - s) + A[r1, c1] * s
        out = top * (1.0 - t) + bot * t
    return np.where(ok, out, np.nan)


def flow_crosscheck(Uf, Vf, Ub, Vb, a, b):
    """-> dict: mask, err (float32 planes), err64, kept_mask, defined_mask, kept, defined, mean (math.fsum), max."""
    Uf, Vf, Ub, Vb = (np.asarray(x, F32) for x in (Uf, Vf, Ub, Vb))
    nrows, ncols = Uf.shape
    uf, vf = Uf.astype(F64), Vf.astype(F64)
    xq = np.arange(1, ncols + 1, dtype=F64)[None, :] + uf
    yq = np.arange(1, nrows + 1, dtype=F64)[:, None] + vf
    ub, vb = sample_xy(Ub, xq, yq), sample_xy(Vb, xq, yq)
    with np.errstate(invalid="ignore", over="ignore"):
        ru, rv = uf + ub, vf + vb
        e = ru * ru + rv * rv
        lim = a * ((uf * uf + vf * vf) + (ub * ub + vb * vb)) + b
        defined = np.isfinite(e)
        kept = defined & (e <= lim)
        err64 = np.sqrt(e)
        err = err64.astype(F32)
    out = dict(mask=kept.astype(F32), err=err, err64=err64, kept_mask=kept, defined_mask=defined)
    out.update(_stats(kept, defined, err64))
    return out
