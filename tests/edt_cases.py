"""Seeded, read-only cases of the distance-transform tests (test_edt_ref.py, test_gpu_edt.py).  Everything is MATLAB-shaped
[nrows, ncols(, frames)], float32, column-major.

Shapes: one pixel, a single row, a single column, 3 x 3, a wide and a tall sliver, a plane that is no multiple of anything, exactly
one wave per column (64 x 64), one past a wave and a workgroup each way (65 x 257), and one of many workgroups (270 x 480), used once.

A mask kind says WHERE the features are; plane(shape, kind, mode) dresses the mask in values whose predicate under `mode` gives
exactly that mask, laced with everything the predicates must tell apart: NaN, +-Inf, +-0.0, subnormals, negative values."""
import functools

import numpy as np

import edt_ref
import interp_cases
import interp_ref

F32 = np.float32

SMALL_SHAPES = [(1, 1), (1, 70), (70, 1), (3, 3), (5, 90), (131, 6), (37, 53), (64, 64), (65, 257)]
BIG_SHAPE = (270, 480)
KINDS = ["empty", "full", "corner_tl", "corner_tr", "corner_bl", "corner_br", "centre", "pair", "quad", "full_row", "full_col", "diagonal",
         "checker", "rand50", "rand5", "rand05", "splat"]
MAX_DISTS = (0, 1, 3, 1000)          # unbounded, the two smallest bands, one larger than every frame here
BASE_MODES = (edt_ref.POSITIVE, edt_ref.NONNEG, edt_ref.NOT_NAN)
TIE_CASE = ((64, 64), "checker")     # every pixel off the board has two to four nearest features
FRAME_CASES = (((37, 53), ("rand5", "empty", "quad")), ((65, 257), ("checker", "corner_br", "full_col")), ((1, 70), ("rand50", "full", "centre")))

_FEATURE = {edt_ref.POSITIVE: (1.0, np.inf, 1e-40, 3e38, 0.5),
            edt_ref.NONNEG: (0.0, -0.0, 1e-40, np.inf, 2.0),
            edt_ref.NOT_NAN: (0.0, -0.0, np.inf, -np.inf, 1e-40, -1e-40, -7.0, 5.0)}
_OTHER = {edt_ref.POSITIVE: (0.0, -0.0, np.nan, -np.inf, -1e-40, -2.5),
          edt_ref.NONNEG: (np.nan, -1e-40, -np.inf, -3.0),
          edt_ref.NOT_NAN: (np.nan,)}


def shape_id(s):
    return "%dx%d" % s


def _frozen(a, dtype=F32):
    a = np.asfortranarray(np.asarray(a, dtype=dtype))
    a.setflags(write=False)
    return a


def has_kind(shape, kind):
    return kind != "splat" or shape in interp_cases.SMALL_SHAPES


def cases():
    """(shape, kind) of every small case."""
    return [(s, k) for s in SMALL_SHAPES for k in KINDS if has_kind(s, k)]


def case_id(c):
    return "%s-%s" % (shape_id(c[0]), c[1])


@functools.lru_cache(maxsize=None)
def mask(shape, kind):
    """The boolean feature mask [nrows, ncols]; read-only."""
    nrows, ncols = shape
    rng = np.random.default_rng([41, nrows, ncols, KINDS.index(kind)])
    i, j = np.meshgrid(np.arange(nrows), np.arange(ncols), indexing="ij")
    M = np.zeros(shape, bool)
    even = lambda n: (n - 1) - (n - 1) % 2           # the last index at an even distance from 0: the bisector is a whole line of pixels
    if kind == "empty":
        pass
    elif kind == "full":
        M[...] = True
    elif kind.startswith("corner_"):
        M[0 if kind[7] == "t" else nrows - 1, 0 if kind[8] == "l" else ncols - 1] = True
    elif kind == "centre":
        M[nrows // 2, ncols // 2] = True
    elif kind == "pair":                              # the column half-way between them ties from top to bottom
        M[nrows // 2, 0] = M[nrows // 2, even(ncols)] = True
    elif kind == "quad":                              # the middle row and the middle column tie, their crossing four ways
        for r in (0, even(nrows)):
            for c in (0, even(ncols)):
                M[r, c] = True
    elif kind == "full_row":
        M[nrows // 2, :] = True
    elif kind == "full_col":
        M[:, ncols // 2] = True
    elif kind == "diagonal":
        M[i == j] = True
    elif kind == "checker":
        M[(i + j) % 2 == 0] = True
    elif kind in ("rand50", "rand5", "rand05"):
        M[rng.random(shape) < {"rand50": 0.5, "rand5": 0.05, "rand05": 0.005}[kind]] = True
    elif kind == "splat":                             # what a splat leaves known: the expanding field opens a regular grid of holes
        Uf, Vf, _, _ = interp_cases.field(shape, "expand")
        Ut, _, _, _ = interp_ref.flow_splat(Uf, Vf, 0.5)
        M[...] = ~np.isnan(Ut)
    else:
        raise ValueError(kind)
    M.setflags(write=False)
    return M


@functools.lru_cache(maxsize=None)
def plane(shape, kind, base_mode):
    """A float32 plane whose features under `base_mode` are mask(shape, kind): the values of both sides cycle through the specials."""
    M = mask(shape, kind)
    rng = np.random.default_rng([43, shape[0], shape[1], KINDS.index(kind), base_mode])
    feat, other = np.array(_FEATURE[base_mode], F32), np.array(_OTHER[base_mode], F32)
    A = np.where(M, feat[rng.integers(0, feat.size, size=shape)], other[rng.integers(0, other.size, size=shape)])
    return _frozen(A)


@functools.lru_cache(maxsize=None)
def frames(shape, kinds, base_mode):
    """Frames with different masks, [nrows, ncols, len(kinds)]."""
    return _frozen(np.stack([plane(shape, k, base_mode) for k in kinds], axis=2))


@functools.lru_cache(maxsize=None)
def sparse_map(shape, kind):
    """A sparse map: numbers on mask(shape, kind) -- with -0.0 and +-Inf among them -- and NaN elsewhere."""
    M = mask(shape, kind)
    rng = np.random.default_rng([47, shape[0], shape[1], KINDS.index(kind)])
    D = rng.normal(size=shape).astype(F32)
    special = np.array([-0.0, np.inf, -np.inf, 0.0], F32)
    pick = rng.random(shape) < 0.2
    D = np.where(pick, special[rng.integers(0, 4, size=shape)], D)
    return _frozen(np.where(M, D, F32(np.nan)))


@functools.lru_cache(maxsize=None)
def want(shape, kind, complement, max_dist):
    """(d2, idx, dist) of the separable restatement for mask(shape, kind) or its complement; read-only, shared by the tests."""
    M = mask(shape, kind)
    A = np.where(M != complement, F32(1.0), F32(0.0))
    return tuple(_frozen(a, a.dtype) for a in edt_ref.edt(A, edt_ref.POSITIVE, max_dist))


@functools.lru_cache(maxsize=None)
def want_frames(shape, kinds, complement, max_dist):
    outs = [want(shape, k, complement, max_dist) for k in kinds]
    return tuple(_frozen(np.stack([o[n] for o in outs], axis=2), outs[0][n].dtype) for n in range(3))
