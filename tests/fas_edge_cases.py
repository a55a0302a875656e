"""The inputs of the FAS stage tests (tests/test_gpu_fas_edges.py), each chosen for one way a stage kernel of csrc/pdeip_fas.hpp can go
wrong, and the functions that say what a case contains.  tests/test_fas_edge_cases.py proves on the CPU that every case is what its
name says.  Arrays are MATLAB-shaped float32 [rows, cols(, C)], built once per process and read-only."""
import functools
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32

BLOCK_ROWS = 256          # PDEIP_PIXEL_INDEX: one workgroup takes 256 rows of one column
TILE_ROWS, TILE_COLS = 64, 4   # k_fas_prepare's tile (FP_TR x FP_TC)
B1, B2, ALPHA = 0.03, 0.97, 0.035

MIN = ((3, 3), (3, 4), (4, 3))                      # check_dims admits nothing smaller; the coarse side is 2
TILE = ((63, 3), (64, 4), (65, 5), (129, 9))        # the prepare tile: one short, exact, one over on each axis, a third tile row
WG = ((257, 3), (511, 4), (512, 3), (513, 5))       # input / output row counts either side of 256 and 512, both parities
GROUPS = dict(MIN=MIN, TILE=TILE, WG=WG)
SHAPES = MIN + TILE + WG
TAIL_SHAPES = ((3, 3), (4, 3), (65, 5), (64, 4), (513, 5), (512, 3))   # one odd and one even shape of each group
TAIL = 64                 # sentinel floats after the last element of an output
VALUE_SHAPE, VALUE_C = (12, 13), 2
ORDER_SHAPE, ORDER_C = (65, 5), 5
SEAM_DRIVER_SHAPE, SEAM_DRIVER_C = (259, 23), 2     # scales 259x23, 130x12, 65x6


@functools.lru_cache(maxsize=None)
def matlab_side():
    spec = importlib.util.spec_from_file_location("matlab_side", os.path.join(ROOT, "oracle", "matlab_side.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _ro(a):
    a = np.asfortranarray(a, dtype=F32)
    a.setflags(write=False)
    return a


def tag(shape):
    return "%dx%d" % tuple(shape)


def half(n):
    return (n + 1) // 2


def coarse(shape):
    return half(shape[0]), half(shape[1])


def channels(shape):
    return {(65, 5): 5, (257, 3): 2}.get(tuple(shape), 1)


# ---- what a shape hits, by index arithmetic ----------------------------------------------------------------------------------------

def last_tile(shape):
    """(rows, cols) of k_fas_prepare's last tile along either axis."""
    return (shape[0] - 1) % TILE_ROWS + 1, (shape[1] - 1) % TILE_COLS + 1


def all_tiles_full(shape):
    return last_tile(shape) == (TILE_ROWS, TILE_COLS)


def row_blocks(nrows):
    return (nrows + BLOCK_ROWS - 1) // BLOCK_ROWS


def down_last_tap(n):
    """The largest input index the last output of fas_down asks for along an axis of n: 2i + 2 at i = ceil(n/2) - 1."""
    return 2 * (half(n) - 1) + 2


def restrict_last_tap(n):
    """The same for fas_restrict: 2i + 1."""
    return 2 * (half(n) - 1) + 1


def reads_past_the_end(stage, A, axis):
    """With the statement alone: does the last output of `stage` along `axis` read a clamped tap?  Two more rows (columns) of other
    values are appended; a tap that was clamped to the last one now finds them, a tap inside the plane does not."""
    A = np.asarray(A, dtype=F32)
    n = A.shape[axis]
    more = list(A.shape)
    more[axis] = 2
    ext = np.concatenate([A, np.full(more, 1000.0, F32)], axis=axis)
    last = half(n) - 1
    a, b = np.take(stage(A), last, axis=axis), np.take(stage(ext), last, axis=axis)
    return not np.array_equal(a.view(np.uint32), b.view(np.uint32))


def differs_from_neighbours(I):
    """Every pixel of every frame differs from its four neighbours."""
    I = I if I.ndim == 3 else I[:, :, None]
    return bool((I[1:, :, :] != I[:-1, :, :]).all() and (I[:, 1:, :] != I[:, :-1, :]).all())


def footprint(A):
    """(number of NaN, number of +-Inf) of a plane or stack."""
    return int(np.isnan(A).sum()), int(np.isinf(A).sum())


def subnormal(A):
    """Non-zero values below the smallest normal single."""
    A = np.asarray(A, dtype=F32)
    return (A != 0) & (np.abs(A) < np.finfo(F32).tiny)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------

def _noise(rng, lo, hi, *shape):
    return rng.uniform(lo, hi, shape).astype(F32)


@functools.lru_cache(maxsize=None)
def frames(shape, C=None):
    """Two frames [rows, cols, C] of independent uniform noise in 0..255: an index that is off by one changes bits."""
    C = channels(shape) if C is None else C
    rng = np.random.default_rng(1000 * shape[0] + 10 * shape[1] + C)
    return _ro(_noise(rng, 0, 255, shape[0], shape[1], C)), _ro(_noise(rng, 0, 255, shape[0], shape[1], C))


@functools.lru_cache(maxsize=None)
def fields(shape):
    """What the stages of a shape take besides the frames: a flow U, V in [-2, 2], a stack A in [-1, 1] for the right-hand side, and
    coarse planes Uc, Ur in [-1, 1] at (ceil(r/2), ceil(c/2))."""
    rng = np.random.default_rng(7 * shape[0] + shape[1])
    cs = coarse(shape)
    return dict(U=_ro(_noise(rng, -2, 2, *shape)), V=_ro(_noise(rng, -2, 2, *shape)), A=_ro(_noise(rng, -1, 1, shape[0], shape[1], channels(shape))),
                Uc=_ro(_noise(rng, -1, 1, *cs)), Ur=_ro(_noise(rng, -1, 1, *cs)))


def upscale_targets(shape):
    """Output sizes of fas_upscale from the coarse plane of `shape`: the driver's two ratios, equal size, one axis unchanged, and for
    the smallest planes a large ratio (first = floor(x) - 1 is negative for many outputs)."""
    cr, cc = coarse(shape)
    out = [tuple(shape), (2 * cr, 2 * cc), (cr, cc), (cr, 2 * cc)]
    if tuple(shape) in MIN:
        out.append((200, 7))
    return list(dict.fromkeys(out))


@functools.lru_cache(maxsize=None)
def order_frames():
    """ORDER_SHAPE with ORDER_C channels, the second frame the first plus N(0, 4) noise: gd then differs from frame to frame by
    orders of magnitude, and the sum over the frames depends on its order."""
    rng = np.random.default_rng(6505)
    I0 = _noise(rng, 0, 255, *ORDER_SHAPE, ORDER_C)
    I1 = (I0 + rng.normal(0.0, 4.0, I0.shape).astype(F32)).astype(F32)
    return _ro(I0), _ro(I1)


def sum3_reversed(A):
    acc = A[:, :, -1].astype(F32)
    for c in range(A.shape[2] - 2, -1, -1):
        acc = (acc + A[:, :, c]).astype(F32)
    return np.asfortranarray(acc)


# non-finite pixels: (row, col, channel, frame 0 or 1, value); five or more pixels apart, two or more off the border
INTERIOR_PIXELS = ((2, 2, 0, 0, np.nan), (2, 8, 0, 0, np.inf), (8, 5, 1, 1, -np.inf))
CORNER_PIXELS = ((0, 0, 0, 0, np.nan), (0, 12, 0, 0, np.inf), (11, 0, 1, 1, -np.inf), (11, 12, 1, 0, np.inf))


def _planted(pixels, seed=1213):
    rng = np.random.default_rng(seed)
    I = [_noise(rng, 0, 255, *VALUE_SHAPE, VALUE_C), _noise(rng, 0, 255, *VALUE_SHAPE, VALUE_C)]
    for r, c, ch, f, v in pixels:
        I[f][r, c, ch] = v
    return _ro(I[0]), _ro(I[1])


@functools.lru_cache(maxsize=None)
def nonfinite_frames(where):
    """'interior': one NaN, one +Inf and one -Inf pixel with whole 5x5 footprints; 'corners': the same in the four corners, where the
    clamp cuts the footprint; 'nan', 'posinf': the first / second interior pixel alone; 'clean': none."""
    pixels = dict(interior=INTERIOR_PIXELS, corners=CORNER_PIXELS, nan=INTERIOR_PIXELS[:1], posinf=INTERIOR_PIXELS[1:2], clean=())[where]
    return _planted(pixels)


@functools.lru_cache(maxsize=None)
def subnormal_frames(scale):
    """Noise frames in 0..255 times `scale` (1e-41: the frames and the derivative planes are subnormal; 1e-20: the products are)."""
    I0, I1 = nonfinite_frames("clean")
    return _ro((I0.astype(np.float64) * scale).astype(F32)), _ro((I1.astype(np.float64) * scale).astype(F32))


SUBNORMAL_SCALES = (1e-41, 1e-20)


@functools.lru_cache(maxsize=None)
def value_fields():
    """For VALUE_SHAPE and the 'clean' frames: their planes; a flow in [-2, 2]; the same with one NaN in U; a huge U (OPnorm overflows
    to Inf at some pixels, gd == +0 there) with its gd, and the gd of k = 0 (Inf everywhere); R, A stacks for the right-hand side
    with R + A == 0 at two of the pixels where the huge flow's gd is zero (0/0) and at one where it is not."""
    ms = matlab_side()
    rng = np.random.default_rng(77)
    U, V = _noise(rng, -2, 2, *VALUE_SHAPE), _noise(rng, -2, 2, *VALUE_SHAPE)
    Unan = U.copy()
    Unan[5, 6] = np.nan
    Uhuge = np.full(VALUE_SHAPE, 1e20, F32)
    planes = ms.fas_prepare(*nonfinite_frames("clean"), B1, B2)
    with np.errstate(over="ignore", divide="ignore"):
        gd_huge = ms.fas_gd(planes, Uhuge, V, B1, B2, ALPHA)
        gd_k0 = ms.fas_gd(planes, U, V, B1, B2, 0.0)
    R, A = _noise(rng, -1, 1, *VALUE_SHAPE, VALUE_C), _noise(rng, -1, 1, *VALUE_SHAPE, VALUE_C)
    cancel = [tuple(p) for p in np.argwhere(gd_huge == 0)[:2]] + [tuple(np.argwhere(gd_huge != 0)[0])]
    for p in cancel:
        R[p] = -A[p]
    return dict(planes=planes, U=_ro(U), V=_ro(V), Unan=_ro(Unan), Uhuge=_ro(Uhuge), gd_huge=_ro(gd_huge), gd_k0=_ro(gd_k0), R=_ro(R), A=_ro(A),
                nan_at=(5, 6), cancel=tuple(cancel))


# (NaN, Inf) counts of the statement's outputs for single planted pixels and for the three interior ones together
FOOTPRINTS = {
    "nan": dict(gauss5=(25, 0), Idt=(1, 0), Idx=(25, 0), Idy=(25, 0), Idxx=(25, 0), Idyy=(25, 0), Idxy=(25, 0), Idxt=(25, 0), Idyt=(25, 0), M=(25, 0),
                Cu=(25, 0), Cv=(25, 0), Du=(25, 0), Dv=(25, 0)),
    # the zero centre tap of HS_D1F: 0 * Inf = NaN in the middle column (row) of a derivative's footprint
    "posinf": dict(gauss5=(0, 25), Idt=(0, 1), Idx=(5, 20), Idy=(5, 20), Idxx=(0, 25), Idyy=(0, 25), Idxy=(9, 16), Idxt=(5, 20), Idyt=(5, 20),
                   M=(9, 16), Cu=(20, 5), Cv=(20, 5), Du=(9, 16), Dv=(9, 16)),
    "interior": dict(gauss5=(25, 25), Idt=(1, 2), Idx=(35, 40), Idy=(35, 40), Idxx=(25, 50), Idyy=(25, 50), Idxy=(43, 32), Idxt=(35, 40),
                     Idyt=(35, 40), M=(43, 32), Cu=(60, 15), Cv=(60, 15), Du=(43, 32), Dv=(43, 32)),
}
