"""Cases of TV-L1 optical flow (tests/tvl1_ref.py, csrc/pdeip_tvl1.hip): the small planes of the stage tests with their parameter sets,
the synthetic pairs of the level and driver tests and the Yosemite pair.  Everything is seeded; expected results are computed once per
case and handed out read-only."""
import functools
import os

import numpy as np

import tvl1_ref

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TILE = (32, 16)             # rows x columns of k_tvl1_block's tile (csrc/pdeip_tvl1.hpp: TILE_R, TILE_C)
T = 4                       # the longest block; the iteration counts are placed around it and around 2
DEFAULT_T = 2               # the library's choice of block length (csrc/pdeip_tvl1.hip)
FORMS = (1, 2, 4)           # the kernel forms PDEIP_TVL1_STEPS selects: single steps, blocks of 2 and of 4
SHAPES = [(1, 1), (1, 70), (70, 1), (2, 2), (3, 5)] + [(r, c) for r in (31, 32, 33) for c in (15, 16, 17)] + [(67, 131)]
ITERS = sorted({0, 1, 2, T - 1, T, T + 1, 2 * T + 3} | {2 * 2 + 3})    # around T = 4, and 2T + 3 of the block of 2
HOLES = ("none", "corner", "seam", "scattered", "all")


def shape_id(shape):
    return "%dx%d" % shape


def _ro(*arrays):
    out = tuple(np.asfortranarray(a, dtype=F32) for a in arrays)
    for a in out:
        a.setflags(write=False)
    return out


def punch(a, holes):
    """NaN into the plane a: 'corner' (a block at the first corner), 'seam' (a block across the tile seams at row 32 and column 16 where
    the plane reaches them, otherwise its centre), 'scattered' (every seventh pixel), 'all'."""
    rows, cols = a.shape
    if holes == "corner":
        a[:max(1, rows // 4), :max(1, cols // 4)] = np.nan
    elif holes == "seam":
        ci, cj = (TILE[0] if rows > TILE[0] + 2 else rows // 2), (TILE[1] if cols > TILE[1] + 2 else cols // 2)
        a[max(0, ci - 3):ci + 3, max(0, cj - 3):cj + 3] = np.nan
    elif holes == "scattered":
        a.reshape(-1)[::7] = np.nan
    elif holes == "all":
        a[:] = np.nan
    return a


@functools.lru_cache(maxsize=None)
def planes(shape, seed=5, holes="none", inf=False):
    """-> rc, gx, gy, U, V, P (four planes) of one stage case, read-only: a linearisation with image-like gradients, a patch with
    gx = gy = 0 (the g2 > 0 branch), NaN in rc by `holes`, +-Inf in rc with `inf`; a flow of a few pixels; duals inside the unit ball."""
    rng = np.random.default_rng(seed + 17 * shape[0] + shape[1])
    rows, cols = shape
    gx, gy = rng.normal(0.0, 0.08, shape), rng.normal(0.0, 0.08, shape)
    gx[rows // 3:rows // 3 + 4, cols // 2:cols // 2 + 3] = 0.0
    gy[rows // 3:rows // 3 + 4, cols // 2:cols // 2 + 3] = 0.0
    gx[-1, -1] = gy[-1, -1] = 0.0
    rc = punch(rng.normal(0.0, 0.05, shape).astype(F32), holes)
    if inf:
        flat = rc.reshape(-1)
        flat[flat.size // 3], flat[flat.size // 2], flat[-1] = np.inf, -np.inf, np.inf
    U, V = rng.uniform(-2.0, 2.0, shape), rng.uniform(-2.0, 2.0, shape)
    P = rng.uniform(-0.45, 0.45, (4,) + shape)
    P[0, -1, :] = P[2, -1, :] = 0.0     # px is zero on the last row, py on the last column, as every call leaves them
    P[1, :, -1] = P[3, :, -1] = 0.0
    return _ro(rc, gx, gy, U, V) + (_ro(*P),)


def param_sets():
    """(lam, huber, iter, holes, inf, with_P): every iteration count, huber 0 and 0.05, lambda 0 and 1e4, every hole pattern, +-Inf, the
    duals given and not."""
    sets = []
    for n, it in enumerate(ITERS):
        sets.append((15.0 if n % 3 else 40.0, 0.0 if n % 2 else 0.05, it, HOLES[n % 5], False, n % 2 == 0))
    top = ITERS[-1]
    sets += [(0.0, 0.0, top, "corner", False, True), (1.0e4, 0.0, top, "scattered", False, False), (1.0e4, 0.05, T + 1, "seam", False, True),
             (15.0, 0.0, top, "none", True, False), (15.0, 0.05, T + 1, "all", True, True), (0.0, 0.05, 1, "none", False, True),
             (15.0, 0.0, 1, "seam", False, False)]
    return sets


@functools.lru_cache(maxsize=None)
def case(shape, pset, seed=5):
    """-> (rc, gx, gy, U, V, P or None), (u, v, four duals): the inputs of a parameter set on a shape and the restated result."""
    lam, huber, it, holes, inf, with_P = pset
    rc, gx, gy, U, V, P = planes(shape, seed, holes, inf)
    state = tvl1_ref.iterate(rc, gx, gy, U, V, tvl1_ref.Consts(lam, huber), it, P if with_P else None)
    want = _ro(state[0], state[1], *state[4:])
    return (rc, gx, gy, U, V, P if with_P else None), want


@functools.lru_cache(maxsize=None)
def rc_case(shape, seed=23):
    """-> I0, W (NaN along one edge and scattered), gx, gy, U0, V0, rc of the rc stage."""
    rng = np.random.default_rng(seed + shape[0] * 31 + shape[1])
    I0, W, gx, gy, U0, V0 = (rng.uniform(-1.0, 1.0, shape).astype(F32) for _ in range(6))
    W[:, -1] = np.nan
    W.reshape(-1)[::5] = np.nan
    gx.reshape(-1)[::11] = np.nan
    return _ro(I0, W, gx, gy, U0, V0, tvl1_ref.rc_stage(I0, W, gx, gy, U0, V0))


# ---- pairs of frames ------------------------------------------------------------------------------------------------------------------
def texture(shape, seed):
    """A smooth random texture in 0..255, float64, [rows, cols] sampled from a function, so that it can be shifted by a fraction."""
    rng = np.random.default_rng(seed)
    k = rng.uniform(0.08, 0.5, (12, 2))
    ph, amp = rng.uniform(0.0, 2 * np.pi, 12), rng.uniform(0.3, 1.0, 12)

    def at(y, x):
        s = sum(a * np.sin(ky * y + kx * x + p) for (ky, kx), p, a in zip(k, ph, amp))
        return 127.5 + 110.0 * s / amp.sum()
    return at


@functools.lru_cache(maxsize=None)
def shifted_pair(shape, du=1.3, dv=-0.7, seed=41):
    """Iin [rows, cols, 2], 0..255: frame 1 is frame 0 moved by (du, dv), so the true flow is constant."""
    rows, cols = shape
    y, x = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing="ij")
    at = texture(shape, seed)
    (I,) = _ro(np.stack([at(y, x), at(y - dv, x - du)], axis=2))
    return I


@functools.lru_cache(maxsize=None)
def yosemite():
    """-> Iin [rows, cols, 2] (0..255), Utrue, Vtrue."""
    d = np.load(os.path.join(ROOT, "tests", "data", "yosemite.npz"))
    (I,) = _ro(d["I"][:, :, :2])
    return I, d["Utrue"], d["Vtrue"]


@functools.lru_cache(maxsize=None)
def yosemite_outliers():
    """The pair with 5 % of frame 1 replaced by uniform noise in 0..255 (default_rng(11))."""
    I = np.array(yosemite()[0])
    rng = np.random.default_rng(11)
    bad = rng.random(I.shape[:2]) < 0.05
    I[:, :, 1][bad] = rng.uniform(0.0, 255.0, I.shape[:2]).astype(F32)[bad]
    return _ro(I)[0]


def errors(U, V, Ut, Vt):
    """AEE over all pixels, AEE below the cloud band, the correlations with the true U and V."""
    epe = np.sqrt((U - Ut) ** 2 + (V - Vt) ** 2)
    return (float(epe.mean()), float(epe[90:, :].mean()), float(np.corrcoef(U.ravel(), Ut.ravel())[0, 1]),
            float(np.corrcoef(V.ravel(), Vt.ravel())[0, 1]))


def within_yosemite_bounds(e):
    """The bounds tests/test_yosemite.py sets for the late-linearisation driver."""
    return e[0] < 0.5 and e[1] < 0.2 and e[2] > 0.9 and e[3] > 0.85


@functools.lru_cache(maxsize=None)
def yosemite_flow(oracle_module, outliers=False):
    """The restated driver on the Yosemite pair with the defaults (on the outlier pair: lambda 10), read-only."""
    I = yosemite_outliers() if outliers else yosemite()[0]
    return _ro(*tvl1_ref.flow_tvl1(oracle_module, I, **(dict(lam=10.0) if outliers else {})))


@functools.lru_cache(maxsize=None)
def small_flow(oracle_module, shape=(40, 52), **param):
    return _ro(*tvl1_ref.flow_tvl1(oracle_module, shifted_pair(shape), **param))
