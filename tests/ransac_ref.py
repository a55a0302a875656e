"""NumPy / plain-Python restatement of SurfaceEquation as include/pdeip.h defines it (the RANSAC fit of a first- or second-order
polynomial surface; mex/source/SurfaceEquation.c + mex/source/library/ransac.c), operation for operation.

`fit` is the definition of the least-squares step: plain loops over Python floats (IEEE float64, no FMA).  `fit_many` performs the
same scalar operations on numpy float64 arrays, one lane per hypothesis (numpy's elementwise multiply, add, divide and sqrt are
the same correctly rounded operations), and tests/test_ransac_ref.py pins the two to each other bit for bit.  Errors are numpy
float32 operations in the stated order; the per-hypothesis sum is float64 in ascending row order (the library's fixed order
differs: errsum agrees within 2*ndata*2^-53 relative, everything else bit for bit)."""
import math

import numpy as np

F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
M64 = (1 << 64) - 1


def splitmix64(x):
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample_sets(seed, iter, n, ndata):
    """uint32 [iter, n]: sample k of hypothesis i is (uint32)(((splitmix64(seed + i*n + k) >> 32) * ndata) >> 32)."""
    out = np.zeros((max(iter, 0), n), np.uint32)
    for i in range(max(iter, 0)):
        for k in range(n):
            out[i, k] = ((splitmix64((seed + i * n + k) & M64) >> 32) * ndata) >> 32
    return out


def _div(a, b):
    """IEEE division of Python floats (Python raises on a zero divisor)."""
    if b == 0.0:
        if a == 0.0 or a != a:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def fit64(As, Bs):
    """Least-squares solution of the [n x ncoef] single sample system As * x = Bs by Householder QR in float64, no pivoting,
    every sum in ascending index.  Returns (x as a list of Python floats, singular)."""
    n, nc = As.shape
    R = [[float(As[i, c]) for c in range(nc)] + [float(Bs[i])] for i in range(n)]  # column nc: the right-hand side
    singular = False
    for k in range(nc):
        s = 0.0
        for i in range(k, n):
            s = s + R[i][k] * R[i][k]
        norm = math.sqrt(s)
        if norm == 0.0:
            singular = True
        alpha = -norm if R[k][k] > 0.0 else norm
        v = [0.0] * n
        v[k] = R[k][k] - alpha
        for i in range(k + 1, n):
            v[i] = R[i][k]
        vtv = 0.0
        for i in range(k, n):
            vtv = vtv + v[i] * v[i]
        for c in range(k + 1, nc + 1):
            dot = 0.0
            for i in range(k, n):
                dot = dot + v[i] * R[i][c]
            f = _div(2.0 * dot, vtv)
            for i in range(k, n):
                R[i][c] = R[i][c] - f * v[i]
        R[k][k] = alpha
    x = [0.0] * nc
    for k in range(nc - 1, -1, -1):
        t = R[k][nc]
        for j in range(k + 1, nc):
            t = t - R[k][j] * x[j]
        x[k] = _div(t, R[k][k])
    return x, singular


def fit(As, Bs):
    """fit64 rounded to single: (float32 [ncoef], singular); a singular system has the zero model."""
    x, singular = fit64(As, Bs)
    if singular:
        return np.zeros(len(x), F32), True
    with np.errstate(over="ignore", invalid="ignore"):
        return np.array(x, np.float64).astype(F32), False


def fit_many(As, Bs):
    """`fit` on [h, n, ncoef] and [h, n] at once: the same operations in the same order, one lane per hypothesis."""
    h, n, nc = As.shape
    R = np.concatenate([As.astype(np.float64), Bs.astype(np.float64)[:, :, None]], axis=2)
    R = [[R[:, i, c].copy() for c in range(nc + 1)] for i in range(n)]
    singular = np.zeros(h, bool)
    with np.errstate(all="ignore"):
        for k in range(nc):
            s = np.zeros(h)
            for i in range(k, n):
                s = s + R[i][k] * R[i][k]
            norm = np.sqrt(s)
            singular |= norm == 0.0
            alpha = np.where(R[k][k] > 0.0, -norm, norm)
            v = [None] * n
            v[k] = R[k][k] - alpha
            for i in range(k + 1, n):
                v[i] = R[i][k]
            vtv = np.zeros(h)
            for i in range(k, n):
                vtv = vtv + v[i] * v[i]
            for c in range(k + 1, nc + 1):
                dot = np.zeros(h)
                for i in range(k, n):
                    dot = dot + v[i] * R[i][c]
                f = (2.0 * dot) / vtv
                for i in range(k, n):
                    R[i][c] = R[i][c] - f * v[i]
            R[k][k] = alpha
        x = [None] * nc
        for k in range(nc - 1, -1, -1):
            t = R[k][nc]
            for j in range(k + 1, nc):
                t = t - R[k][j] * x[j]
            x[k] = t / R[k][k]
        M = np.stack(x, axis=1).astype(F32)
    M[singular] = 0
    return M, singular


def errors(A, B, m, singular=False):
    """e[j] = (A[j,:] . m - B[j])^2 in single: t = A[j,0]*m[0]; t = t + A[j,1]*m[1]; ...; d = t - B[j]; e = d*d."""
    if singular:
        return np.full(A.shape[0], FLT_MAX, F32)
    m = np.asarray(m, F32).reshape(-1)
    with np.errstate(all="ignore"):
        t = A[:, 0] * m[0]
        for c in range(1, A.shape[1]):
            t = t + A[:, c] * m[c]
        d = t - B
        return d * d


def abs_min_of(min_set_size, ndata):
    v = F32(F32(min_set_size) * F32(ndata)) + F32(0.5)
    return 0 if v < 1 else (0xFFFFFFFF if v >= 4294967296.0 else int(v))


def score(e, thr2):
    inl = e <= thr2  # a NaN error is never an inlier
    acc = np.cumsum(e[inl].astype(np.float64))  # sequential, ascending row order
    return int(inl.sum()), (float(acc[-1]) if acc.size else 0.0)


def select(counts, sums, abs_min, given=None):
    """RANSAC()'s rules (ransac.c:112-211) on score lists.  counts, sums: per hypothesis, in order; given: (count, sum) of the
    given model or None.  Returns (winner, margins): winner is -1 for the given model, an index, or None (nothing to return);
    margins lists (h, sum, best_sum, best) of every `sum < best_sum` comparison made with enough inliers (best: the holder of
    best_sum, -1 the given model, None nobody yet)."""
    best_sum, best, found, best_inlr, inlr = FLT_MAX, None, False, 0, None
    margins = []
    if given is not None and given[0] >= abs_min:
        best_sum, best, found = given[1], -1, True
    for h, (c, s) in enumerate(zip(counts, sums)):
        if c >= abs_min:
            margins.append((h, s, best_sum, best))
        if c >= abs_min and s < best_sum:
            found, best, best_sum = True, h, s
        elif c >= best_inlr and not found:
            best_inlr, inlr = c, h
    w = best if found else inlr
    if w is None and given is not None:
        w = -1
    return w, margins


def surface_equation(A, B, M_in, err_thr, min_set_size, iter, seed=None, sets=None):
    """Returns a dict: M [ncoef] float32, err [ndata] float32, inliers int [iter+1] ([0]: the given model's, -1 if none), errsum
    float64 [iter+1], winner (-1: the given model), models [iter, ncoef], singular [iter], margins (see select)."""
    A = np.asarray(A, F32)
    B = np.asarray(B, F32).reshape(-1)
    ndata, nc = A.shape
    n = nc + 1
    iter = max(int(iter), 0)
    thr2 = F32(err_thr) * F32(err_thr)
    if sets is None:
        sets = sample_sets(seed, iter, n, ndata)
    sets = np.asarray(sets, np.uint32).reshape(iter, n)
    if iter:
        models, singular = fit_many(A[sets], B[sets])
    else:
        models, singular = np.zeros((0, nc), F32), np.zeros(0, bool)
    given = None
    inliers, errsum = [-1], [0.0]
    if M_in is not None:
        given = score(errors(A, B, M_in), thr2)
        inliers, errsum = [given[0]], [given[1]]
    for h in range(iter):
        c, s = score(errors(A, B, models[h], singular[h]), thr2)
        inliers.append(c)
        errsum.append(s)
    w, margins = select(inliers[1:], errsum[1:], abs_min_of(min_set_size, ndata), given)
    if w is None:
        raise ValueError("no hypotheses and no given model")
    M = np.asarray(M_in, F32).reshape(-1) if w == -1 else models[w]
    err = errors(A, B, M, False if w == -1 else singular[w])
    return dict(M=M.copy(), err=err, inliers=np.array(inliers, np.int64), errsum=np.array(errsum), winner=w, models=models,
                singular=singular, margins=margins)


def design(X, Y, order):
    """single([X Y 1]) or single([X.^2 Y.^2 X.*Y X Y 1]) of double coordinate vectors."""
    X = np.asarray(X, np.float64)
    Y = np.asarray(Y, np.float64)
    one = np.ones_like(X)
    cols = [X, Y, one] if order == 1 else [X * X, Y * Y, X * Y, X, Y, one]
    return np.stack(cols, axis=1).astype(F32)


def masked_data(PHI, D, order):
    """A, B of the pixels with PHI >= 0 in column-major order: X = j + 1, Y = i + 1 (DispSegmentation.m:329-343)."""
    with np.errstate(invalid="ignore"):
        mask = np.asarray(PHI) >= 0
    jj, ii = np.nonzero(mask.T)  # column-major rank
    return design(jj + 1, ii + 1, order), np.asarray(D, F32)[ii, jj]


def dist_plane(D, M, order, singular=False):
    """The error formula on every pixel's row against D (FLT_MAX everywhere when the chosen hypothesis is singular)."""
    nrows, ncols = D.shape
    jj, ii = np.meshgrid(np.arange(ncols), np.arange(nrows))
    e = errors(design(jj.T.ravel() + 1, ii.T.ravel() + 1, order), np.asarray(D, F32).T.ravel(), M, singular)
    return np.asfortranarray(e.reshape(ncols, nrows).T)


def surface_fit_masked(PHI, D, order, M_in, err_thr, min_set_size, iter, seed=None, sets=None):
    """(result dict of surface_equation or None for an empty mask, M_out, dist plane, ndata)."""
    A, B = masked_data(PHI, D, order)
    nc = 3 if order == 1 else 6
    if A.shape[0] == 0:
        M = np.asarray(M_in, F32).reshape(-1) if M_in is not None else np.full(nc, np.nan, F32)
        return None, M, dist_plane(D, M, order), 0
    r = surface_equation(A, B, M_in, err_thr, min_set_size, iter, seed=seed, sets=sets)
    w = r["winner"]
    return r, r["M"], dist_plane(D, r["M"], order, w >= 0 and bool(r["singular"][w])), A.shape[0]
