"""Seeded cases of the frame-interpolation tests (test_interp_ref.py, test_gpu_interp.py): small fields at the shapes where the
kernels' indexing can go wrong, and the 96 x 128 scene with its ground truth.  Everything is float32, column-major, MATLAB-shaped
[nrows, ncols(, C)].

Shapes: the smallest plane the calls accept, a wide and a tall sliver, a plane that is no multiple of anything, exactly one wave per
column, one past a wave and a workgroup in each direction (65 x 257), and one of many workgroups (270 x 480)."""
import functools

import numpy as np

from crosscheck_cases import lace_positions

F32, F64 = np.float32, np.float64

SMALL_SHAPES = [(3, 3), (5, 90), (131, 6), (37, 53), (64, 64), (65, 257)]
BIG_SHAPE = (270, 480)
KINDS = ["zero", "shift_even", "shift_odd", "normal", "expand", "contract", "layers", "nonfinite", "neg_zero", "edges", "all_nonfinite"]
T_LOW, T_HALF, T_HIGH = 2.0 ** -20, 0.5, 1.0 - 2.0 ** -20
SHIFT_EVEN, SHIFT_ODD = (2.0, -2.0), (1.0, 3.0)     # (u, v): t u integer at t = 0.5, and not


def shape_id(s):
    return "%dx%d" % s


def _frozen(a):
    a = np.asfortranarray(np.asarray(a, dtype=F32))
    a.setflags(write=False)
    return a


def _flat(A):
    return A.reshape(-1, order="F")


def _lace(A, values, at):
    f = _flat(A)
    for k, p in enumerate(at):
        f[p] = values[k % len(values)]


def channels_of(shape):
    """1 or 3, alternating over the shapes."""
    return 3 if (SMALL_SHAPES + [BIG_SHAPE]).index(shape) % 2 else 1


def images(shape, channels, seed=0):
    """Two textured frames in 0..1, [nrows, ncols, channels]."""
    nrows, ncols = shape
    rng = np.random.default_rng([17, nrows, ncols, channels, seed])
    jj, ii = np.meshgrid(np.arange(ncols), np.arange(nrows))
    out = []
    for f in range(2):
        planes = [0.5 + 0.25 * np.sin(0.37 * ii + 0.9 * ch + f) * np.cos(0.29 * jj - 0.5 * ch) + 0.2 * rng.random(shape) for ch in range(channels)]
        out.append(np.stack(planes, axis=2))
    return out


def landing_edges(shape, axis, step=1):
    """Displacements d with 0.5 d exact: the landing at t = 0.5 is exactly on the last line, exactly on the first, and d one float32
    ulp beyond each (the landing then lies just outside, its floor or floor + 1 is dropped), by (i + step j) % 4."""
    rows, cols = shape
    i, j = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    pos = (j if axis == 1 else i).astype(F32)
    last = F32(cols if axis == 1 else rows)
    to_last, to_first = F32(2) * (last - (pos + F32(1))), F32(-2) * pos
    kind = (i + step * j) % 4
    d = np.where(kind == 0, to_last, np.where(kind == 1, to_first, np.where(kind == 2, np.nextafter(to_last, F32(np.inf)),
                                                                            np.nextafter(to_first, F32(-np.inf)))))
    return d.astype(F32)


@functools.lru_cache(maxsize=None)
def field(shape, kind):
    """-> Uf, Vf, I0, I1 (frames [nrows, ncols, C], C = channels_of(shape)); read-only."""
    nrows, ncols = shape
    C = channels_of(shape)
    rng = np.random.default_rng([23, nrows, ncols, KINDS.index(kind)])
    I0, I1 = images(shape, C)
    i, j = np.meshgrid(np.arange(nrows), np.arange(ncols), indexing="ij")
    x, y = (j + 1).astype(F64), (i + 1).astype(F64)
    cx, cy = float((ncols + 1) // 2), float((nrows + 1) // 2)
    U = np.zeros(shape, F32, order="F")
    V = np.zeros(shape, F32, order="F")
    at = lace_positions(shape)
    if kind == "zero":
        pass
    elif kind in ("shift_even", "shift_odd"):
        u, v = SHIFT_EVEN if kind == "shift_even" else SHIFT_ODD
        U[...], V[...] = u, v
    elif kind == "normal":
        U[...], V[...] = 2.0 * rng.normal(size=shape), 2.0 * rng.normal(size=shape)
    elif kind == "expand":            # scale 4 about the centre at t = 0.5, 2.5 at t = 0.25: more than the 2 x 2 targets of a landing cover
        U[...], V[...] = 6.0 * (x - cx), 6.0 * (y - cy)
    elif kind == "contract":          # at t = 0.5 every source lands exactly on (cx, cy): one key for all
        U[...], V[...] = 2.0 * (cx - x), 2.0 * (cy - y)
    elif kind == "layers":            # the left half moves right, the right half left; frame 1 agrees with the left half only
        d = 2
        U[...] = np.where(j < ncols // 2, d, -d)
        I1 = np.empty_like(I0)
        I1[:, d:, :] = I0[:, :-d, :]
        I1[:, :d, :] = I0[:, :d, :]
    elif kind == "nonfinite":
        U[...], V[...] = 2.0 * rng.normal(size=shape), 2.0 * rng.normal(size=shape)
        _lace(U, [np.nan, np.inf, -np.inf], at)
        _lace(V, [-np.inf, np.nan, 1.0], at[::2])
        U[rng.random(shape) < 0.1] = np.nan
        I1[:, :, 0].flat[::13] = np.nan        # a NaN sample: the cost is +Inf, the source still splats
        I0[:, :, C - 1].flat[5::29] = np.inf
    elif kind == "neg_zero":
        U[...], V[...] = rng.integers(-1, 2, size=shape), rng.integers(-1, 2, size=shape)
        U[rng.random(shape) < 0.4] = -0.0
        V[rng.random(shape) < 0.4] = -0.0
        _lace(U, [-0.0], at)
        _lace(V, [-0.0, 0.0], at)
    elif kind == "edges":
        U[...], V[...] = landing_edges(shape, 1), landing_edges(shape, 0, step=2)   # every pairing of the four kinds occurs
    elif kind == "all_nonfinite":
        U[...] = np.nan
        V[...] = 1.0
        _lace(U, [np.inf, -np.inf, 1.0], at)
        _lace(V, [1.0, 2.0, np.nan], at)
    else:
        raise ValueError(kind)
    return _frozen(U), _frozen(V), _frozen(I0), _frozen(I1)


@functools.lru_cache(maxsize=None)
def masks(shape):
    """Two 0 / 1 planes with every pairing, one entry a NaN and one a 2 (both count as passed: != 0)."""
    rng = np.random.default_rng([29, shape[0], shape[1]])
    M0, M1 = (rng.random(shape) < 0.6).astype(F32), (rng.random(shape) < 0.6).astype(F32)
    M0[0, 0], M1[-1, -1] = np.nan, 2.0
    return _frozen(M0), _frozen(M1)


def cases():
    """(shape, kind, t, with_images) of the kernel tests: every kind on every small shape at t = 0.5, the extreme times where the
    landing barely leaves the source or nearly reaches the target, the contraction also without costs, one big plane."""
    out = [(s, k, T_HALF, True) for s in SMALL_SHAPES for k in KINDS]
    for s in ((37, 53), (65, 257)):
        out += [(s, k, t, True) for k in ("zero", "shift_odd", "normal") for t in (T_LOW, T_HIGH)]
    out += [(s, "contract", T_HALF, False) for s in SMALL_SHAPES]
    out += [((37, 53), "normal", T_HALF, False), (BIG_SHAPE, "normal", T_HALF, True)]
    return out


def case_id(c):
    return "%s-%s-t%.7g-%s" % (shape_id(c[0]), c[1], c[2], "cost" if c[3] else "index")


# ---- the scene: a textured square moving 6 px to the right over a static textured background -----------------------------------------
SCENE_SHAPE = (96, 128)
SQUARE = (30, 66, 40, 76)      # rows r0:r1, columns c0:c1 of the square in frame 0
MOVE = 6


def _background(ii, jj):
    return 0.45 + 0.2 * np.sin(0.35 * ii) * np.cos(0.27 * jj) + 0.1 * np.sin(0.11 * (ii + 2 * jj))


def _square_texture(ii, jj):
    """The square's own pattern in its own coordinates."""
    return 0.55 + 0.3 * np.cos(0.8 * ii) * np.sin(0.6 * jj)


def _render(shift):
    nrows, ncols = SCENE_SHAPE
    jj, ii = np.meshgrid(np.arange(ncols, dtype=F64), np.arange(nrows, dtype=F64))
    r0, r1, c0, c1 = SQUARE
    inside = (ii >= r0) & (ii < r1) & (jj >= c0 + shift) & (jj < c1 + shift)
    return np.where(inside, _square_texture(ii - r0, jj - c0 - shift), _background(ii, jj)), inside


@functools.lru_cache(maxsize=None)
def scene():
    """-> I0, I1, Imid (the true frame at t = 0.5, rendered, not interpolated), Uf, Vf, Ub, Vb (the true flows), valid (the pixels
    away from the border).  One channel."""
    I0, in0 = _render(0)
    I1, in1 = _render(MOVE)
    Imid, _ = _render(MOVE // 2)
    Uf, Ub = np.where(in0, float(MOVE), 0.0), np.where(in1, -float(MOVE), 0.0)
    zero = np.zeros(SCENE_SHAPE)
    valid = np.zeros(SCENE_SHAPE, bool)
    valid[4:-4, 8:-8] = True
    return tuple(_frozen(a) for a in (I0, I1, Imid, Uf, zero, Ub, zero)) + (valid,)


def rms(A, truth, where):
    d = (np.asarray(A, F64) - np.asarray(truth, F64))[where]
    return float(np.sqrt(np.mean(d * d)))
