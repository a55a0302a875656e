"""Inputs shared by tests/test_fit_batch.py (CPU: the conditions on the fixtures) and tests/test_gpu_fit_batch.py (GPU: the batched
masked fit against S single calls and against the restatement).  Every case's restatement result is computed once
(functools.lru_cache) and never modified.

Planes: 37x53 (1961 pixels: seven full 256-pixel blocks and a remainder, odd nrows), 64x80 (exactly 20 blocks), 176x192 (33 792
pixels: from 32 768 on a score tile has 1024 rows, four per thread)."""
import functools

import numpy as np

import ransac_cases as rc
import ransac_batch_ref as bref

F32 = np.float32
ERR_THR, MIN_SET = 0.1, 0.3


def _flat(nrows, ncols, f):
    """A plane from its pixels in memory (column-major) order."""
    return np.asarray(f, np.float64).reshape(ncols, nrows).T


def mask(name, nrows, ncols):
    npix = nrows * ncols
    ii, jj = np.meshgrid(np.arange(nrows), np.arange(ncols), indexing="ij")
    f = -np.ones(npix)
    if name == "full":
        f[:] = 1
    elif name == "empty":
        pass
    elif name == "one":
        f[777] = 1
    elif name == "b256":        # exactly one block's worth of pixels, ending on a block edge
        f[512:768] = 1
    elif name == "b257":        # ... and one pixel into the next block
        f[512:769] = 1
    elif name == "stripe_small":
        return np.where(jj < 2, 1.0, -1.0)
    elif name == "stripe_mid":
        return np.where((jj >= 2) & (jj < 10), 1.0, -1.0)
    elif name == "stripe_big":
        return np.where(jj >= 10, 1.0, -1.0)
    elif name == "nan_laced":
        rng = np.random.default_rng(nrows * 1000 + ncols + 1)
        f = rng.uniform(-1, 1, npix)
        f[rng.random(npix) < 0.2] = np.nan
    elif name == "negzero":     # PHI == 0 counts, with either sign
        f[3 * nrows:5 * nrows:2] = 0.0
        f[3 * nrows + 1:5 * nrows:2] = -0.0
    elif name == "blob":
        return 0.3 * min(nrows, ncols) - np.hypot(ii - 0.45 * nrows, jj - 0.55 * ncols)
    elif name == "checker":
        return np.where((ii + jj) % 2 == 0, 1.0, -1.0)
    else:
        raise KeyError(name)
    return _flat(nrows, ncols, f)


# neighbouring segments differ; two identical planes (blob) stand at s = 4 and s = 11
SEVENTEEN = ("full", "empty", "one", "b256", "blob", "b257", "stripe_small", "stripe_big", "stripe_mid", "nan_laced", "negzero", "blob",
             "checker", "empty", "full", "one", "nan_laced")

# name -> dict(shape, masks, order, iter, given, alias (M_out is M_in), seed, stride, nan_d)
CASES = {}


def _add(name, shape, masks, order, iter, given, seed, alias=False, stride=65536, nan_d=False):
    CASES[name] = dict(shape=shape, masks=tuple(masks), order=order, iter=iter, given=given, alias=alias, seed=seed, stride=stride, nan_d=nan_d)


_add("s1_37x53_o1", (37, 53), ("nan_laced",), 1, 10, False, 101)
_add("s3_37x53_o2_alias", (37, 53), ("full", "empty", "one"), 2, 10, True, 102, alias=True)
_add("s17_37x53_o1_given", (37, 53), SEVENTEEN, 1, 10, True, 103)
_add("s17_37x53_o2", (37, 53), SEVENTEEN, 2, 10, False, 104)
_add("s3_37x53_o1_nan_d", (37, 53), ("full", "nan_laced", "negzero"), 1, 10, True, 105, nan_d=True)
_add("s3_37x53_o1_stride0", (37, 53), ("blob", "stripe_mid", "blob"), 1, 10, False, 106, stride=0)
_add("s3_37x53_o2_wrap", (37, 53), ("blob", "checker", "stripe_big"), 2, 10, False, 2 ** 64 - 3, stride=2 ** 63 + 1)  # the seed sum wraps
_add("s3_64x80_o1_i100", (64, 80), ("b256", "b257", "stripe_big"), 1, 100, False, 107)
_add("s3_64x80_o2_i100_alias", (64, 80), ("stripe_small", "full", "one"), 2, 100, True, 108, alias=True)
_add("s17_64x80_o2_i0", (64, 80), SEVENTEEN, 2, 0, True, 109)
_add("s17_64x80_o1_alias", (64, 80), SEVENTEEN, 1, 10, True, 110, alias=True)
_add("s3_176x192_o1", (176, 192), ("full", "stripe_small", "nan_laced"), 1, 10, True, 111)
_add("s2_176x192_o2", (176, 192), ("blob", "empty"), 2, 10, False, 112)


@functools.lru_cache(maxsize=None)
def case(name):
    """(PHI [nrows, ncols, S], D, M_in [ncoef, S] or None, case dict, restatement tuple of ransac_batch_ref.surface_fit_masked_batch)."""
    c = CASES[name]
    nrows, ncols = c["shape"]
    PHI = np.asfortranarray(np.stack([mask(m, nrows, ncols) for m in c["masks"]], axis=2).astype(F32))
    D = rc.two_planes(nrows, ncols, seed=c["seed"] % 1000, noise=0.02)
    if c["nan_d"]:
        D = D.copy()
        D[np.random.default_rng(5).random(D.shape) < 0.03] = np.nan
    M_in = None
    if c["given"]:
        base = np.array(rc.PLANE2000 if c["order"] == 1 else (0, 0, 0) + rc.PLANE2000, np.float64)
        M_in = np.stack([base * (1.001 + 0.0005 * s) for s in range(len(c["masks"]))], axis=1).astype(F32)
    want = bref.surface_fit_masked_batch(PHI, D, c["order"], M_in, ERR_THR, MIN_SET, c["iter"], seed=c["seed"], seed_stride=c["stride"])
    for x in (PHI, D) + (() if M_in is None else (M_in,)):
        x.setflags(write=False)
    return PHI, D, M_in, c, want


def all_margins():
    """[(case name and segment, restatement result, given model)] of every segment with data of every case the GPU tests run."""
    out = []
    for name in CASES:
        _, _, M_in, _, want = case(name)
        for s, r in enumerate(want[0]):
            if r is not None:
                out.append(("%s[%d]" % (name, s), r, None if M_in is None else M_in[:, s]))
    return out
