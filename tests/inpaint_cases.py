"""Seeded cases of the hole-filling tests (test_inpaint_ref.py, test_gpu_inpaint.py): the 96 x 128 scene, and the small planes and
hole patterns the stage kernels are compared on.  Everything is float32, column-major, MATLAB-shaped [nrows, ncols(, F)]."""
import functools

import numpy as np

F32 = np.float32
NAN = F32(np.nan)


def _frozen(a):
    a = np.asfortranarray(a.astype(F32))
    a.setflags(write=False)
    return a


# ---- the scene: a slanted background, a rectangle 10 px nearer, 13 % holes ------------------------------------------------------------
SCENE_SHAPE = (96, 128)
RECT = (slice(28, 70), slice(48, 92))      # the foreground
BAND = (slice(28, 70), slice(38, 48))      # the 10-px occlusion band left of it: background that view 1 does not see


@functools.lru_cache(maxsize=None)
def scene():
    """-> truth, sparse (NaN holes), guide (an image in 0..1 with the rectangle's edge), band mask."""
    nrows, ncols = SCENE_SHAPE
    jj, ii = np.meshgrid(np.arange(ncols), np.arange(nrows))
    truth = 20.0 + 0.02 * jj + 0.02 * ii
    truth[RECT] += 10.0
    guide = 0.35 + 0.04 * np.sin(0.31 * ii) * np.cos(0.23 * jj)
    guide[RECT] += 0.4
    rng = np.random.default_rng(1013)
    hole = rng.random(SCENE_SHAPE) < 0.05
    hole[BAND] = True
    hole[:, :6] = True
    band = np.zeros(SCENE_SHAPE, bool)
    band[BAND] = True
    sparse = np.where(hole, np.nan, truth)
    return _frozen(truth), _frozen(sparse), _frozen(guide), band


def rms(A, truth, where):
    d = (np.asarray(A, np.float64) - np.asarray(truth, np.float64))[where]
    return float(np.sqrt(np.mean(d * d)))


# ---- planes of the stage tests ---------------------------------------------------------------------------------------------------------
RESIZE_SHAPES = (((37, 53), (28, 40)), ((5, 90), (4, 68)), ((131, 6), (99, 5)), ((8, 8), (4, 4)))
HOLE_KINDS = ("none", "random", "first_col_last_row", "empty_frame")


def smooth_plane(shape, seed, frames=None):
    """A smooth field of both signs plus a little noise; frames=None: a plane."""
    nrows, ncols = shape
    rng = np.random.default_rng([seed, nrows, ncols])
    jj, ii = np.meshgrid(np.arange(ncols), np.arange(nrows))
    F = frames or 1
    P = np.stack([3.0 * np.sin(0.21 * ii + 0.4 * f) * np.cos(0.17 * jj - 0.3 * f) + 0.02 * (ii - jj) + 0.05 * rng.standard_normal(shape)
                  for f in range(F)], axis=2)
    return np.asfortranarray((P if frames else P[:, :, 0]).astype(F32))


@functools.lru_cache(maxsize=None)
def holed(shape, kind):
    """The sparse map of one (shape, kind).  empty_frame: F = 2, an all-NaN frame beside a full one; otherwise one plane."""
    rng = np.random.default_rng([7, shape[0], shape[1], HOLE_KINDS.index(kind)])
    if kind == "empty_frame":
        D = smooth_plane(shape, 3, frames=2)
        D[:, :, 0] = NAN
        return _frozen(D)
    D = smooth_plane(shape, 3)
    if kind == "random":
        D[rng.random(shape) < 0.3] = NAN
    elif kind == "first_col_last_row":
        D[:, 0] = NAN
        D[-1, :] = NAN
    return _frozen(D)


@functools.lru_cache(maxsize=None)
def tie_plane():
    """8 x 8 halved to 4 x 4: output column o has the four column taps 2o-1 .. 2o+2 (clamped) of weights 1/8, 3/8, 3/8, 1/8, all
    exact, and the same four row taps.  With columns 1, 2, 5, 6 holes, outputs 0 and 2 know their left two taps and outputs 1 and 3
    their right two (neighbouring outputs share taps, so not all four can know the left two): den = 1/8 + 3/8 = 0.5 exactly."""
    D = smooth_plane((8, 8), 11)
    D[:, [1, 2, 5, 6]] = NAN
    return _frozen(D)


@functools.lru_cache(maxsize=None)
def single_known(shape, frames=2):
    D = np.full(shape + (frames,), NAN, F32)
    for f in range(frames):
        D[(3 + 5 * f) % shape[0], (2 + 7 * f) % shape[1], f] = F32(-1.5 + 4.0 * f)
    return _frozen(D)


ASSEMBLE_CASES = (((37, 53), 1, 0), ((40, 48), 3, 3), ((5, 90), 2, 1), ((131, 6), 1, 1))   # shape, F, guide channels
ASSEMBLE_HOLES = ("none", "random", "one_frame", "corners")


@functools.lru_cache(maxsize=None)
def assemble_case(shape, F, G, holes):
    """-> X (no NaN), D (sparse), guide or None; [nrows, ncols, F] throughout (F = 1 keeps the third axis)."""
    rng = np.random.default_rng([9, shape[0], shape[1], F, ASSEMBLE_HOLES.index(holes)])
    X = smooth_plane(shape, 5, frames=F)
    D = (X + 0.1 * rng.standard_normal(X.shape)).astype(F32)
    D.flat[::17] = X.flat[::17]                      # X == D exactly somewhere: psi = 1/sqrt(eps)
    if holes == "random":
        D[rng.random(D.shape) < 0.3] = NAN
    elif holes == "one_frame":
        D[:, :, F - 1][rng.random(shape) < 0.3] = NAN
    elif holes == "corners":
        for i, j in ((0, 0), (0, -1), (-1, 0), (-1, -1)):
            D[i, j, :] = NAN
    guide = None if G == 0 else _frozen(np.stack([0.5 + 0.4 * np.tanh(0.3 * (smooth_plane(shape, 20 + g) - 0.5)) for g in range(G)], axis=2))
    return _frozen(X), _frozen(D), guide


@functools.lru_cache(maxsize=None)
def level_case(F, with_guide):
    """One 56 x 72 level, 20 % holes including a 9-px band: -> D (sparse), X0 (the estimate entering the level), guide or None."""
    shape = (56, 72)
    rng = np.random.default_rng([31, F, int(with_guide)])
    jj, ii = np.meshgrid(np.arange(72), np.arange(56))
    base = [(0.5 + 0.4 * np.sin(0.2 * ii + f) * np.cos(0.15 * jj) + 0.3 * (ii > 28)) for f in range(F)]
    truth = np.stack(base, axis=2).astype(F32)
    D = truth.copy()
    hole = rng.random(truth.shape) < 0.13
    hole[:, 30:39, :] = True
    D[hole] = NAN
    X0 = np.where(hole, F32(0.5), D).astype(F32)
    guide = (0.3 + 0.5 * (ii > 28) + 0.02 * np.sin(0.4 * jj)).astype(F32) if with_guide else None
    sq = (lambda a: a[:, :, 0]) if F == 1 else (lambda a: a)
    return _frozen(sq(D)), _frozen(sq(X0)), None if guide is None else _frozen(guide)
