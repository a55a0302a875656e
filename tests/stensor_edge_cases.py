"""Cases for the stage kernels of structure-tensor anisotropic diffusion (csrc/pdeip_stensor.hpp, pdeip_tensor8.hpp), chosen from
the constants of the kernels and the rules of include/pdeip.h and not from image content: the shapes at which the last 64 x 4 tile
of k_st_weights is full, one line long, or ends on the wrap position; tensors J on which the rule's exp returns exactly 0 or
exactly 1, so that only correctly rounded operations remain and the weights can be compared bit for bit; J with a NaN or an Inf; the
channel counts and the call sequence that size the workspace slots; the Gaussian on mixed signs, wide binades and subnormals.
tests/test_stensor_edge_cases.py proves on the CPU that each case reaches what it claims; tests/test_gpu_stensor_edges.py runs them.
Arrays are [rows, cols(, planes)], read-only, column-major as the device holds them."""
import functools
import math
import zlib

import numpy as np

import stensor_ref as ref

F32, F64 = np.float32, np.float64

# name: (value, the line it mirrors)
CONSTANTS = {
    "GAUSS_T": (64, "csrc/pdeip_stensor.hpp: constexpr int GAUSS_RMAX = 32, GAUSS_T = 64, GAUSS_WAVES = 4;"),
    "GAUSS_WAVES": (4, "csrc/pdeip_stensor.hpp: constexpr int GAUSS_RMAX = 32, GAUSS_T = 64, GAUSS_WAVES = 4;"),
    "GAUSS_RMAX": (32, "csrc/pdeip_stensor.hpp: constexpr int GAUSS_RMAX = 32, GAUSS_T = 64, GAUSS_WAVES = 4;"),
    "TT_R": (64, "csrc/pdeip_tensor8.hpp: constexpr int TT_R = 64, TT_C = 4;"),
    "TT_C": (4, "csrc/pdeip_tensor8.hpp: constexpr int TT_R = 64, TT_C = 4;"),
    "PIXEL_BLOCK": (256, "csrc/pdeip_ctx.hpp: pixel_grid(): (nrows + 255) / 256 blocks; csrc/pdeip_stensor.hip launches them with dim3(256)"),
}
GAUSS_T, GAUSS_WAVES, GAUSS_RMAX, TT_R, TT_C, PIXEL_BLOCK = (CONSTANTS[k][0] for k in ("GAUSS_T", "GAUSS_WAVES", "GAUSS_RMAX", "TT_R", "TT_C", "PIXEL_BLOCK"))

MODES = ("ced", "eed")
TAUS = (1.0, 0.37)


def _frozen(a):
    a = np.asfortranarray(np.asarray(a, dtype=F32))
    a.setflags(write=False)
    return a


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def image(seed, shape):
    """The content of tests/test_gpu_stensor.py: 0..255, oblique waves, a step and noise."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(shape[0], dtype=F64), np.arange(shape[1], dtype=F64), indexing="ij")
    planes = []
    for c in range(shape[2] if len(shape) == 3 else 1):
        P = 120 + 70 * np.sin(0.5 * i + 0.3 * j + c) + 40 * (j > shape[1] / 2) + rng.normal(0, 12, shape[:2])
        planes.append(np.clip(P, 0, 255))
    I = np.stack(planes, axis=2) if len(shape) == 3 else planes[0]
    return np.asfortranarray(I.astype(F32))


# ---- the tiles of k_st_weights ---------------------------------------------------------------------------------------------------
# nrows in {3, 63, 64, 65, 128, 129} x ncols in {3, 4, 5, 8, 9}: every row and every column value, and (64, 4) and (65, 5)
SEAM_SHAPES = ((3, 3), (63, 4), (64, 4), (65, 5), (128, 8), (129, 9), (63, 9), (64, 3), (129, 4), (65, 8), (128, 5), (3, 9))
SEAM_ROWS, SEAM_COLS = (3, 63, 64, 65, 128, 129), (3, 4, 5, 8, 9)


def last_tile(n, T):
    """(tiles, lines of the frame in the last tile, position of the last halo line of the last tile) along an axis of n lines tiled by
    T.  The halo of tile k spans k T - 1 .. k T + T; position n is the wrap position (it reads line 0), positions beyond it are
    skipped by st_tile_fill."""
    tiles = (n + T - 1) // T
    first = (tiles - 1) * T
    return tiles, n - first, first + T


def halo_ends_on_wrap(n, T):
    return last_tile(n, T)[2] == n


@functools.lru_cache(maxsize=None)
def seam_J(shape, mode):
    """J [rows, cols, 3] of the image content at the mode's default scales, by the restatement alone."""
    p = ref.params(mode)
    return _frozen(ref.structure_tensor(image(_seed("seam", shape) % 1000, shape), p["sigma"], p["rho"]))


def frame_masks(shape):
    """Per weight (W NW N NE E SE S SW) the positions TVdenoise8's assembly zeroes."""
    m = [np.zeros(shape, bool) for _ in range(8)]
    for k in (0, 1, 7):
        m[k][:, 0] = True
    for k in (3, 4, 5):
        m[k][:, -1] = True
    for k in (1, 2, 3):
        m[k][0, :] = True
    for k in (5, 6, 7):
        m[k][-1, :] = True
    return m


def dominance_slack(TRACE, w8):
    """TRACE - sum |w_k| + 9 x 2^-24 x TRACE in float64 from the float32 planes: >= 0 where the row is weakly diagonally dominant
    to the nine single roundings of its entries."""
    T = np.asarray(TRACE, F32).astype(F64)
    return T - sum(np.abs(np.asarray(w, F32).astype(F64)) for w in w8) + 9 * 2.0 ** -24 * T


# ---- saturated J: the exp of the rule returns exactly 0 or exactly 1 ----------------------------------------------------------------
SAT_SHAPES = ((65, 9), (129, 5))
LOW_E, HIGH_E = (-40, -6), (31, 100)
FIXED_ANGLES = (0.0, math.pi / 4, math.pi / 2, 3 * math.pi / 4)
SAT_FAMILIES = ("low", "high", "mixed", "special")


def _oriented(rng, shape, kind):
    """(j11, j12, j22) = m (cos^2 t, cos t sin t, sin^2 t) rounded to single, m = 2^e; the first pixels of column 0 and the last of
    the last column take the fixed angles."""
    t = rng.uniform(0.0, math.pi, shape)
    t[:4, 0] = FIXED_ANGLES
    t[-4:, -1] = FIXED_ANGLES
    lo, hi = LOW_E if kind == "low" else HIGH_E
    m = np.exp2(rng.integers(lo, hi + 1, shape).astype(F64))
    c, s = np.cos(t), np.sin(t)
    return np.stack([m * c * c, m * c * s, m * s * s], axis=2).astype(F32)


# (j11, j12, j22) / m: isotropic (r = 0, mu1 > 0); zero; not positive semi-definite: r = 0 with mu1 < 0, j12^2 > j11 j22 (mu1 = 3 m),
# a negative j11 with mu1 = m, both eigenvalues negative with r = 2 m
SPECIAL_TRIPLES = ((1.0, 0.0, 1.0), (0.0, 0.0, 0.0), (-1.0, 0.0, -1.0), (1.0, 2.0, 1.0), (-1.0, 1.0, 0.5), (-3.0, 0.0, -1.0))
SPECIAL_ROWS, SPECIAL_COLS = (0, 1, 31, 62, 63, 64), (0, 2, 3, 4)   # where the special pixels sit (rows also counted from the end)


def special_positions(shape):
    rows = sorted({r for r in SPECIAL_ROWS if r < shape[0]} | {shape[0] - 1 - r for r in (0, 1)})
    cols = sorted({c for c in SPECIAL_COLS if c < shape[1]} | {shape[1] - 1})
    return [(r, c) for r in rows for c in cols]


@functools.lru_cache(maxsize=None)
def saturated_J(family, shape):
    rng = np.random.default_rng(_seed("sat", family, shape))
    if family in ("low", "high"):
        return _frozen(_oriented(rng, shape, family))
    low, high = _oriented(rng, shape, "low"), _oriented(rng, shape, "high")
    i, j = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    J = np.where(((i >= TT_R) != (j >= TT_C))[:, :, None], high, low)   # the families meet along row 64 and along column 4
    if family == "special":
        for n, (r, c) in enumerate(special_positions(shape)):
            m = 2.0 ** (HIGH_E[0] + n % 40) if n % 2 else 2.0 ** (LOW_E[0] + n % 30)
            J[r, c] = np.asarray(SPECIAL_TRIPLES[(n // 2) % len(SPECIAL_TRIPLES)], F64) * m
    return _frozen(J)


def uniform_45(shape, m=2.0 ** 40):
    """j = m (cos^2, cos sin, sin^2) at 45 degrees: m (1/2, 1/2, 1/2), exact in single."""
    return _frozen(np.full(shape + (3,), 0.5 * m))


# every bit-for-bit weights case: name -> (J, keyword parameters of the rule)
def saturated_cases():
    cases = {}
    for shape in SAT_SHAPES:
        for family in SAT_FAMILIES:
            cases["%s-%dx%d" % ((family,) + shape)] = (saturated_J(family, shape), {})
    cases["uniform45-65x9"] = (uniform_45((65, 9)), {})
    cases["uniform45-alpha0-65x9"] = (uniform_45((65, 9)), {"alpha": 0.0})
    return cases


def proven_saturated(J, mode, p):
    """Per pixel: no exp is taken, or numpy's exp of the rule's argument is exactly 0.0 or exactly 1.0."""
    taken, value = ref.exp_terms(J, mode, p)
    return ~taken | (value == 0.0) | (value == 1.0)


def rule_params(mode, kw):
    """The restatement's parameters with the case's keywords; those of the other mode's rule are dropped (alpha is CED's)."""
    return ref.params(mode, **{k: v for k, v in kw.items() if k in ref.DEFAULTS[mode]})


# ---- non-finite J -------------------------------------------------------------------------------------------------------------------
NF_SHAPE = (65, 9)
NF_PLACES = {"interior": ((30, 6),), "corner00": ((0, 0),), "corner0E": ((0, 8),), "cornerE0": ((64, 0),), "cornerEE": ((64, 8),),
             "seam63-3": ((63, 3),), "seam64-4": ((64, 4),), "adjacent": ((20, 5), (21, 5))}
WRAP_PLACES = {"last-row": ((64, 5),), "last-column": ((33, 8),), "corner": ((64, 8),)}


def nonfinite_J(value, plane, places):
    """The saturated 'mixed' background with `value` in plane `plane` (0: j11, 1: j12, 2: j22) at `places`."""
    J = np.array(saturated_J("mixed", NF_SHAPE), order="F")
    for (r, c) in places:
        J[r, c, plane] = value
    return _frozen(J)


def neighbourhood(shape, places, reach=1):
    m = np.zeros(shape, bool)
    for (r, c) in places:
        m[max(r - reach, 0):r + reach + 1, max(c - reach, 0):c + reach + 1] = True
    return m


# ---- structure tensor -----------------------------------------------------------------------------------------------------------------
TENSOR_CHANNELS = (2, 4, 5)
TENSOR_SHAPES = ((65, 9), (17, 129))
TENSOR_SCALES = ((0.0, 0.0), (0.7, 0.0), (0.7, 4.0), (1.5, 1.25), (0.0, 10.6))   # the last: R = 32 on the product planes
# (what, shape, channels or frames): one process, in this order
SEQUENCE = (("tensor", (129, 65), 5), ("tensor", (3, 3), 1), ("gauss", (65, 65), 4), ("tensor", (65, 9), 2))
SEQUENCE_SCALES = (0.7, 4.0)
SEQUENCE_SIGMA = 4.0
NF_IMAGE_SHAPE = (70, 40)
NF_IMAGE_PLACES = {"interior": (30, 20), "corner": (0, 0), "seam": (63, 3)}
NF_IMAGE_SCALES = ((0.7, 0.0), (0.7, 4.0))


def nonfinite_image(value, where, channels):
    shape = NF_IMAGE_SHAPE + ((channels,) if channels > 1 else ())
    I = np.array(image(97, shape), order="F")
    I[where + ((channels // 2,) if channels > 1 else ())] = value
    return _frozen(I)


# ---- Gaussian -------------------------------------------------------------------------------------------------------------------------
SIGMA_R1, SIGMA_R32 = 1.0 / 3.0, 32.0 / 3.0
GAUSS_SIGMAS = (0.0, 0.5, 1.25, 4.0, 10.6, SIGMA_R1, SIGMA_R32)
GAUSS_NEW_SHAPES = ((64, 4), (3, 8), (65, 65), (33, 3))
GAUSS_SHAPES = GAUSS_NEW_SHAPES + ((3, 3), (63, 5), (5, 129), (130, 66))
GAUSS_FAMILIES = ("image", "binades", "tiny")


@functools.lru_cache(maxsize=None)
def gauss_input(family, shape, frames):
    full = shape + ((frames,) if frames > 1 else ())
    rng = np.random.default_rng(_seed("gauss", family, shape, frames))
    if family == "image":
        return _frozen(image(sum(shape) + frames, full))
    m = 1.0 + rng.integers(0, 1 << 23, size=full).astype(F64) * 2.0 ** -23   # [1, 2), exact in single
    sign = np.where(rng.integers(0, 2, size=full) == 1, -1.0, 1.0)
    if family == "binades":
        return _frozen(sign * m * np.exp2(rng.integers(-20, 21, size=full).astype(F64)))
    A = (sign * m * 2.0 ** -140).astype(F32)   # subnormal: every product with a tap (< 1) is subnormal too
    A[rng.random(full) < 0.1] = F32(-0.0)
    return _frozen(A)


# ---- one step and the driver ------------------------------------------------------------------------------------------------------------
STEP_SHAPES = ((62, 6), (63, 6), (6, 62), (6, 63))   # the ringed plane is 64 / 65 rows or columns: the solvers' own strip and tile edges
STEP_CHANNELS = (1, 2)
# name: (shape, channels, mode, keyword parameters)
DRIVER_CASES = {
    "channels2": ((17, 33), 2, "ced", dict(iters=3)),
    "channels4": ((65, 9), 4, "eed", dict(iters=2)),
    "omega1.5": ((17, 33), 1, "ced", dict(iters=3, omega=1.5)),
    "tau0.37": ((17, 33), 1, "eed", dict(iters=3, tau=0.37)),
    "iters2.9": ((17, 33), 1, "ced", dict(iters=2.9)),
    "inner0": ((17, 33), 1, "ced", dict(iters=2, inner_iter=0)),
    "alr": ((63, 6), 2, "ced", dict(iters=2, solver=2)),
}
CHAIN = ((63, 6), 2, "ced")
