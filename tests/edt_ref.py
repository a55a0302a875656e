"""The NumPy restatement of the exact Euclidean distance transform of include/pdeip.h (pdeip_edt) and of what stands on it
(pdeip_bwdist, pdeip_signed_distance, pdeip_nearest_fill, pdeip_flow_interpolate_nearest).  Pinned by test_edt_ref.py;
tests/test_gpu_edt.py compares the GPU with it bit for bit.

Two forms of the transform.  edt_brute minimises the key (d2, idx) over ALL features of a frame, so the tie rule -- the lowest
column-major linear index among equidistant features -- is stated, not implied; max_dist is applied to its result.  edt is the
separable form (a column pass, then a minimum over the columns), which restricts the search to the max_dist box as the kernels do;
it is what the one large case and the GPU tests use.  test_edt_ref.py holds the two equal on every small case.

Arrays are MATLAB-shaped [nrows, ncols(, frames)]; indices are 0-based, j * nrows + i, within a frame."""
import numpy as np

import crosscheck_ref as cr
import interp_ref as ir

F32, F64 = np.float32, np.float64
I32_MAX = int(np.iinfo(np.int32).max)
POSITIVE, NONNEG, NOT_NAN, POSITIVE_NOT, NONNEG_NOT, NOT_NAN_NOT = 0, 1, 2, 4, 5, 6
MODES = (POSITIVE, NONNEG, NOT_NAN, POSITIVE_NOT, NONNEG_NOT, NOT_NAN_NOT)
MODE_NAMES = {POSITIVE: "positive", NONNEG: "nonneg", NOT_NAN: "not_nan", POSITIVE_NOT: "positive_not", NONNEG_NOT: "nonneg_not",
              NOT_NAN_NOT: "not_nan_not"}
_SHIFT = 1 << 31     # key = d2 * 2^31 + idx: d2 < 2^31 and idx < 2^31, so the key orders (d2, idx) lexicographically in an int64
_NO_KEY = np.iinfo(np.int64).max


def features(A, mode):
    """The feature mask of the plane(s) A under PDEIP_EDT_* `mode`."""
    A = np.asarray(A, F32)
    with np.errstate(invalid="ignore"):
        base = (A > 0, A >= 0, A == A)[mode & 3]
    return ~base if mode & 4 else base


def _frames(A):
    A = np.asarray(A)
    return A if A.ndim == 3 else A[:, :, None]


def limit(d2, idx, max_dist):
    """(d2, idx, dist) of an unbounded (d2, idx) under max_dist: a pixel whose nearest feature is farther reports "none"."""
    d2, idx = np.asarray(d2, np.int64), np.asarray(idx, np.int64)
    if max_dist > 0:
        far = d2 > max_dist * max_dist
        d2, idx = np.where(far, I32_MAX, d2), np.where(far, -1, idx)
    with np.errstate(invalid="ignore"):
        dist = np.where(d2 == I32_MAX, F32(np.inf), np.sqrt(d2.astype(F64)).astype(F32)).astype(F32)
    return np.asfortranarray(d2.astype(np.int32)), np.asfortranarray(idx.astype(np.int32)), np.asfortranarray(dist)


def _outputs(key, max_dist):
    """(d2, idx, dist) of a plane of keys."""
    none = key == _NO_KEY
    return limit(np.where(none, I32_MAX, key // _SHIFT), np.where(none, -1, key % _SHIFT), max_dist)


def _brute_frame(M, max_dist):
    nrows, ncols = M.shape
    fi, fj = np.nonzero(M)
    fidx = (fj * nrows + fi).astype(np.int64)
    key = np.full((nrows, ncols), _NO_KEY, np.int64)
    if fidx.size:
        # d2 of every pixel to every feature is (i - fi)^2 + (j - fj)^2: the two squares are tabulated once (int32: d2 < 2^31), a
        # column of pixels at a time is their sum; then the smallest d2, and among the features that reach it the smallest index
        fi, fj = fi.astype(np.int32), fj.astype(np.int32)
        ri = (np.arange(nrows, dtype=np.int32)[:, None] - fi[None, :]) ** 2        # [nrows, features]
        cj = (np.arange(ncols, dtype=np.int32)[:, None] - fj[None, :]) ** 2        # [ncols, features]
        for j in range(ncols):
            d2 = ri + cj[j][None, :]
            best = d2.min(axis=1)
            idx = np.where(d2 == best[:, None], fidx[None, :], _SHIFT).min(axis=1)
            key[:, j] = best.astype(np.int64) * _SHIFT + idx
    return _outputs(key, max_dist)


def _separable_frame(M, max_dist):
    nrows, ncols = M.shape
    rows = np.arange(nrows, dtype=np.int64)[:, None]
    far = 1 << 40
    up = np.maximum.accumulate(np.where(M, rows, -far), axis=0)                     # the last feature row at or above
    down = np.minimum.accumulate(np.where(M, rows, far)[::-1], axis=0)[::-1]        # the first feature row at or below
    du, dd = rows - up, down - rows
    g = np.where(du <= dd, -du, dd)                                                 # the upper of two equidistant features
    has = np.minimum(du, dd) < far // 2
    if max_dist > 0:
        has &= np.abs(g) <= max_dist
    cols = np.arange(ncols, dtype=np.int64)[None, :]
    key = np.full((nrows, ncols), _NO_KEY, np.int64)
    for c in range(ncols):
        gc = np.where(has[:, c], g[:, c], 0)[:, None]
        dj = cols - c
        k = (dj * dj + gc * gc) * _SHIFT + (c * nrows + rows + gc)
        ok = has[:, c][:, None] & ((np.abs(dj) <= max_dist) if max_dist > 0 else True)
        key = np.minimum(key, np.where(ok, k, _NO_KEY))
    return _outputs(key, max_dist)


def _per_frame(fn, A, mode, max_dist):
    A = np.asarray(A, F32)
    M = _frames(features(A, mode))
    outs = [fn(M[:, :, f], int(max_dist)) for f in range(M.shape[2])]
    return tuple(np.asfortranarray(np.stack([o[k] for o in outs], axis=2).reshape(A.shape)) for k in range(3))


def edt_brute(A, mode=POSITIVE, max_dist=0):
    """-> d2 (int32), idx (int32), dist (float32): the minimum of (d2, idx) over all features, then max_dist."""
    return _per_frame(_brute_frame, A, mode, max_dist)


def edt(A, mode=POSITIVE, max_dist=0):
    """-> d2 (int32), idx (int32), dist (float32): the separable form, searching the max_dist box only."""
    return _per_frame(_separable_frame, A, mode, max_dist)


def tie_count(A, mode=POSITIVE):
    """Pixels of the plane A that have more than one nearest feature."""
    M = features(A, mode)
    nrows, ncols = M.shape
    fi, fj = (v.astype(np.int64) for v in np.nonzero(M))
    if fi.size == 0:
        return 0
    pi, pj = np.arange(nrows * ncols) % nrows, np.arange(nrows * ncols) // nrows
    count = 0
    step = max(1, (1 << 22) // fi.size)
    for p0 in range(0, nrows * ncols, step):
        d2 = (pi[p0:p0 + step, None] - fi[None, :]) ** 2 + (pj[p0:p0 + step, None] - fj[None, :]) ** 2
        count += int(((d2 == d2.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
    return count


def bwdist(BW):
    """-> D (float32), IDX (int32, 0-based; -1 without a feature)."""
    _, idx, dist = edt(BW, POSITIVE, 0)
    return dist, idx


def signed_distance(A, max_dist=0):
    A = np.asarray(A, F32)
    _, _, to_out = edt(A, NONNEG_NOT, max_dist)
    _, _, to_in = edt(A, NONNEG, max_dist)
    inside = features(A, NONNEG)
    d = np.where(inside, to_out, to_in).astype(F32)
    if max_dist > 0:
        d = np.where(np.isinf(d), F32(float(max_dist) + 1.0), d).astype(F32)
    m = (d - F32(0.5)).astype(F32)
    return np.asfortranarray(np.where(inside, m, -m).astype(F32))


def nearest_fill(D, max_dist=0):
    """-> out, filled, dist (float32 planes like D)."""
    D = np.asarray(D, F32)
    D3 = _frames(D)
    _, idx, dist = edt(D, NOT_NAN, max_dist)
    idx3 = _frames(idx)
    out, filled = D3.copy(), np.zeros(D3.shape, F32)
    for f in range(D3.shape[2]):
        flat = D3[:, :, f].reshape(-1, order="F")
        hole = np.isnan(D3[:, :, f]) & (idx3[:, :, f] >= 0)
        plane = out[:, :, f]
        plane[hole] = flat[idx3[:, :, f][hole]]
        filled[:, :, f][hole] = 1.0
    return np.asfortranarray(out.reshape(D.shape)), np.asfortranarray(filled.reshape(D.shape)), dist


def flow_interpolate_nearest(I0, I1, Uf, Vf, Ub=None, Vb=None, t=0.5, a=0.01, b=0.5, use_costs=1, max_dist=0):
    """-> It, Ut, Vt (the filled flow at t), source: interp_ref.flow_interpolate with the hole filling replaced by one feature
    transform of Ut's holes and a gather of both planes through it; a hole without a source becomes 0."""
    M0 = M1 = None
    if Ub is not None:
        M0 = cr.flow_crosscheck(Uf, Vf, Ub, Vb, a, b)["mask"]
        M1 = cr.flow_crosscheck(Ub, Vb, Uf, Vf, a, b)["mask"]
    Ut, Vt, _, _ = ir.flow_splat(Uf, Vf, t, I0 if use_costs else None, I1 if use_costs else None)
    _, idx, _ = edt(Ut, NOT_NAN, max_dist)
    filled = []
    for P in (Ut, Vt):
        flat = P.reshape(-1, order="F")
        filled.append(np.asfortranarray(np.where(idx >= 0, flat[np.maximum(idx, 0)], F32(0.0)).astype(F32)))
    It, src = ir.interp_blend(I0, I1, filled[0], filled[1], t, M0, M1)
    return It, filled[0], filled[1], src
