"""Cases of primal-dual total variation (tests/tvpd_ref.py, csrc/pdeip_tvpd.hip): the quality scene, the small planes of the GPU tests and
their parameter sets.  Everything is seeded; expected results are computed once per case and handed out read-only."""
import functools

import numpy as np

import tvpd_ref

F32 = np.float32

# ---- the quality scene: piecewise affine, gross outliers, a little noise ----------------------------------------------------------------
SCENE_SHAPE = (96, 128)
# The 20 x 20 hole of the second quality condition lies inside one affine piece (the background, east of the box and short of the
# diagonal).  A hole across a discontinuity also loses where the edge runs, which no data term can bring back, and a first-order method
# moves an edge through 20 pixels without data far more slowly than 300 iterations; what the condition is about -- missing data beside
# outliers -- does not need either.
SCENE_HOLE = (slice(40, 60), slice(92, 112))
ROF_LAMBDAS = (0.05, 0.1, 0.2, 0.5, 1.0)
L1_LAMBDA, QUALITY_ITER = 0.8, 300


@functools.lru_cache(maxsize=None)
def scene(hole=False):
    """-> clean, noisy (float32 [96, 128], read-only): three affine pieces in 0..64 -- a tilted background, a tilted box and the
    half-plane beyond a diagonal --, 10 % of the pixels replaced by uniform outliers in 0..64, N(0, 0.3) on the rest; with `hole` a
    20 x 20 block of the input is NaN."""
    rows, cols = SCENE_SHAPE
    i, j = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing="ij")
    clean = 12.0 + 0.05 * j + 0.03 * i
    box = (i >= 20) & (i < 70) & (j >= 25) & (j < 75)
    clean[box] = (34.0 + 0.12 * (i - 20) - 0.04 * (j - 25))[box]
    far = i + 0.7 * j > 150
    clean[far] = (55.0 - 0.06 * j + 0.02 * i)[far]
    rng = np.random.default_rng(7)
    noisy = clean + rng.normal(0.0, 0.3, clean.shape)
    out = rng.random(clean.shape) < 0.10
    noisy[out] = rng.uniform(0.0, 64.0, clean.shape)[out]
    noisy = noisy.astype(F32)
    if hole:
        noisy[SCENE_HOLE] = np.nan
    clean, noisy = np.asfortranarray(clean.astype(F32)), np.asfortranarray(noisy)
    clean.setflags(write=False)
    noisy.setflags(write=False)
    return clean, noisy


def rms(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return float(np.sqrt(np.mean(d * d)))


@functools.lru_cache(maxsize=None)
def scene_l1(hole=False):
    """TV-L1 of the scene at the quality parameters (read-only)."""
    out = tvpd_ref.tv_pd(scene(hole)[1], "l1", L1_LAMBDA, QUALITY_ITER)
    out.setflags(write=False)
    return out


# ---- the small planes of the GPU tests ---------------------------------------------------------------------------------------------
TILE = (32, 16)             # rows x columns of k_tvpd_block's tile (csrc/pdeip_tvpd.hpp: TILE_R, TILE_C)
BLOCKS = (2, 4, 8)          # the blocked forms PDEIP_TVPD_STEPS selects
DEFAULT_T = 4               # the library's choice
SHAPES = [(1, 1), (1, 70), (70, 1), (2, 2), (3, 3), (3, 5),        # degenerate planes; 3 x 5 is smaller than every halo
          (31, 17), (32, 16), (33, 15), (65, 33), (129, 65),        # one pixel to either side of the tile's edges, in both directions
          (131, 67)]
BIG_SHAPE = (270, 480)


def shape_id(shape):
    return "%dx%d" % shape


def iters_for(T):
    return sorted({0, 1, 2, T - 1, T, T + 1, 2 * T + 3})


def plane(shape, seed, holes="none", frames=1):
    """A data plane [rows, cols(, frames)]: a ramp with a step, N(0, 1) noise and 10 % outliers; holes: 'none', 'corner' (a NaN block at
    the first corner), 'seam' (a NaN block across the tile seams at row 32 and column 16, where the plane reaches them; otherwise its
    centre), 'scattered' (every seventh pixel)."""
    rng = np.random.default_rng(seed)
    rows, cols = shape
    out = []
    for _ in range(frames):
        i, j = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
        a = 0.3 * i + 0.2 * j + 8.0 * (i + j > (rows + cols) // 2) + rng.normal(0.0, 1.0, shape)
        bad = rng.random(shape) < 0.10
        a[bad] = rng.uniform(-20.0, 60.0, shape)[bad]
        a = a.astype(F32)
        if holes == "corner":
            a[:max(1, rows // 4), :max(1, cols // 4)] = np.nan
        elif holes == "seam":
            ci, cj = (TILE[0] if rows > TILE[0] + 2 else rows // 2), (TILE[1] if cols > TILE[1] + 2 else cols // 2)
            a[max(0, ci - 3):ci + 3, max(0, cj - 3):cj + 3] = np.nan
        elif holes == "scattered":
            a.reshape(-1)[::7] = np.nan
        out.append(a)
    res = np.asfortranarray(out[0] if frames == 1 else np.stack(out, axis=2))
    res.setflags(write=False)
    return res


def param_sets(T):
    """The parameter sets every shape runs: (model, lam, huber, iter, holes, frames, given_start).  Between them: both models, huber 0
    and 0.05, every iteration count around the block T, lambda 0 and a large lambda, one and three frames, every hole pattern, a given
    start and the nearest-fill start."""
    its = iters_for(T)
    sets = []
    for n, it in enumerate(its):
        sets.append(("l1" if n % 2 == 0 else "l2", 0.8, 0.0 if n % 3 else 0.05, it, ("none", "corner", "seam", "scattered")[n % 4], 1 + 2 * (n % 2), n % 3 == 1))
    top = its[-1]
    sets += [("l2", 0.3, 0.05, top, "seam", 1, False), ("l1", 0.0, 0.0, top, "corner", 1, True), ("l2", 0.0, 0.05, T + 1, "none", 3, False),
             ("l1", 1.0e4, 0.0, top, "scattered", 1, False), ("l2", 1.0e4, 0.0, T, "none", 1, True), ("l1", 0.8, 0.05, T + 1, "seam", 3, False)]
    return sets


def start_for(shape, frames, seed):
    rng = np.random.default_rng(seed + 1000)
    u0 = np.asfortranarray(rng.uniform(-5.0, 40.0, shape + ((frames,) if frames > 1 else ())).astype(F32))
    u0.setflags(write=False)
    return u0


@functools.lru_cache(maxsize=None)
def case(shape, pset, seed=3):
    """-> f, u0 (or None), want: the inputs of a parameter set on a shape and the restated result (all read-only)."""
    model, lam, huber, it, holes, frames, given = pset
    f = plane(shape, seed, holes, frames)
    u0 = start_for(shape, frames, seed) if given else None
    want = tvpd_ref.tv_pd(f, model, lam, it, huber=huber, u0=u0)
    want.setflags(write=False)
    return f, u0, want
