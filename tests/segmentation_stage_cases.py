"""Inputs that take region competition's stage kernels (csrc/pdeip_segmentation.hpp: k_seg_sizes(_final), k_seg_variance(_final),
k_seg_data, k_seg_label) off their habitual shapes: planes at the seams of the wave, the 256-pixel tile, the batch of 16 tile
partials and the 256 threads of the final passes; segment counts on both sides of 256; values at the edges of the range.  Everything
is generated from fixed seeds and returned read-only; the restatement's results are computed once per process and shared.  What a
case holds is proved on the CPU by tests/test_segmentation_stage_cases.py; tests/test_gpu_segmentation_stages.py consumes the cases.

SEAM_PLANES: (nrows, ncols) -> (tiles, pixels in the last tile, pixels in the last wave), chosen for npix = nrows*ncols:
  2x2                            the smallest plane the refusals admit
  3x21, 2x32, 5x13               63, 64, 65: a wave less a lane, one wave, one wave plus a lane
  5x51, 2x128, 2x129             255, 256, 258: a tile less a pixel, one tile, one tile plus two pixels
  48x80, 15x273, 64x64, 17x241   15 tiles; 16 with 255 pixels in the last; 16; 17 with one pixel in the last: k_seg_variance_final's
                                 batch of 16 is not entered, entered once with no tail, entered once with a one-tile tail
  62x128, 64x128, 3x2731         31, 32, 33 tiles: two batches with a tail of 15, of none, of one
  256x256, 131x501               256 and 257 tiles (the last holds 95 pixels): the second trip of k_seg_sizes_final's stride loop
"""
import functools

import numpy as np

import segmentation_ref as sr

F32 = np.float32
TILE, WAVE, AHEAD = sr.TILE, sr.WAVE, 16

SEAM_PLANES = {
    (2, 2): (1, 4, 4),
    (3, 21): (1, 63, 63), (2, 32): (1, 64, 64), (5, 13): (1, 65, 1),
    (5, 51): (1, 255, 63), (2, 128): (1, 256, 64), (2, 129): (2, 2, 2),
    (48, 80): (15, 256, 64), (15, 273): (16, 255, 63), (64, 64): (16, 256, 64), (17, 241): (17, 1, 1),
    (62, 128): (31, 256, 64), (64, 128): (32, 256, 64), (3, 2731): (33, 1, 1),
    (256, 256): (256, 256, 64), (131, 501): (257, 95, 31),
}
BIG_PLANES = ((256, 256), (131, 501))  # above 65 000 pixels: S in {1, 3} only
MANY_S = (255, 256, 257)               # around the 256 threads of k_seg_variance_final's segment loop
MANY_S_ALL = (5, 13)                   # all four kernels at MANY_S
MANY_S_NO_DATA = (17, 241)             # sizes, variance and label only: the restatement's data term is O(S^2) per pixel
RANGE_PLANES = ((37, 53), (17, 241))
STAGE_S = (1, 2, 3, 17)


def seam_s(shape):
    return (1, 3) if shape in BIG_PLANES else STAGE_S


SEAM_CASES = tuple((shape, S) for shape in SEAM_PLANES for S in seam_s(shape))                  # every kernel
MANY_CASES = tuple((shape, S) for shape in (MANY_S_ALL, MANY_S_NO_DATA) for S in MANY_S)         # sizes, variance, label
DATA_CASES = SEAM_CASES + tuple((MANY_S_ALL, S) for S in MANY_S)


def case_id(c):
    return "%dx%dx%d" % (c[0][0], c[0][1], c[1])


def edges(shape):
    """(first pixel of the last tile, last pixel of the plane), as memory (column-major) positions."""
    npix = shape[0] * shape[1]
    return (-(-npix // TILE) - 1) * TILE, npix - 1


def at(shape, p):
    """Memory position -> (row, column)."""
    return p % shape[0], p // shape[0]


def specials(shape):
    """Memory positions of PHI's NaN, -0.0 and +0.0: the first three that are no edge.  The 2x2 plane has two such pixels only: its
    +0.0 (which counts: 0 >= 0) stands at the first pixel, one of the edges."""
    first, last = edges(shape)
    free = [p for p in range(min(shape[0] * shape[1], 5)) if p not in (first, last)]
    return free[0], free[1], free[2] if len(free) > 2 else first


FIRST_DIST, LAST_DIST, OVER_CAP = F32(2.625), F32(5.375), F32(150.0)


def _frozen(*arrays):
    out = tuple(np.asfortranarray(a) for a in arrays)
    for a in out:
        a.flags.writeable = False
    return out


def _seam(shape, S, seed):
    rng = np.random.default_rng([shape[0], shape[1], S, seed])
    full = shape + (S,)
    PHI = rng.standard_normal(full).astype(F32)
    dist = (rng.standard_normal(full) ** 2 * rng.choice([0.01, 1.0, 80.0], size=full)).astype(F32)
    DH = (rng.random(full) * 0.05).astype(F32)
    first, last = edges(shape)
    nan_at, negz_at, posz_at = specials(shape)
    for p, d in ((first, FIRST_DIST), (last, LAST_DIST)):  # the edges count in every segment, each with a dist of its own
        PHI[at(shape, p) + (slice(None),)] = np.abs(PHI[at(shape, p) + (slice(None),)]) + F32(0.5)
        dist[at(shape, p) + (slice(None),)] = d
    PHI[at(shape, nan_at) + (0,)] = np.nan
    PHI[at(shape, negz_at) + (S - 1,)] = F32(-0.0)
    PHI[at(shape, posz_at) + (0,)] = F32(0.0)
    dist[at(shape, nan_at) + (slice(None),)] = 0               # t = 0, as stage_case has it
    dist[at(shape, negz_at) + (S - 1,)] = OVER_CAP             # counted (-0.0 >= 0) without a cap, left out by the cap of 100
    return PHI, dist, DH


@functools.lru_cache(maxsize=None)
def seam_case(shape, S, seed=0):
    """(PHI, dist, DH) [nrows, ncols, S] after the recipe of segmentation_cases.stage_case: PHI with a NaN, a -0.0 and a +0.0, dist a
    squared residual with values on both sides of 100, DH on both sides of 0.02.  In addition the last pixel of the plane and the first
    pixel of the last tile have PHI >= 0.5 in every segment (2x2: segment 0's +0.0 at the first pixel) and a dist no other pixel of the segment has (FIRST_DIST, LAST_DIST; the
    last pixel's where they are one pixel): an edge element dropped or taken twice shows in n and in the sum."""
    return _frozen(*_seam(shape, S, seed))


VARIANCE_EDGES = ("empty", "plus_inf", "minus_inf", "both_inf")


@functools.lru_cache(maxsize=None)
def variance_edge_case(shape):
    """(PHI, dist) of four segments, each the single-segment seam plane with one change: no pixel inside (n = 0, cov NaN); a +Inf
    dist at the last pixel (cov +Inf without a cap, finite with one); a -Inf dist at the pixel before it, made an inside one (below any
    minCOV: cov = minCOV with or without a cap); both (NaN without a cap, minCOV with one)."""
    P1, d1, _ = _seam(shape, 1, 0)
    PHI, dist = np.repeat(P1, 4, axis=2), np.repeat(d1, 4, axis=2)
    PHI[:, :, 0] = -np.abs(PHI[:, :, 0]) - F32(1)
    last = edges(shape)[1]
    lastp, prev = at(shape, last), at(shape, last - 1)
    PHI[prev + (slice(2, 4),)] = 1
    dist[lastp + (1,)] = np.inf
    dist[prev + (2,)] = -np.inf
    dist[lastp + (3,)] = np.inf
    dist[prev + (3,)] = -np.inf
    return _frozen(PHI, dist)


@functools.lru_cache(maxsize=None)
def label_case(shape, S):
    """PHI [nrows, ncols, S] for the numbered map: every pixel held by one segment drawn at random or by none, a tenth of them by
    a second one too (S >= 2), a zero and a NaN that hold nothing; segment S alone at the plane's last pixel; two segments at the
    first pixel of the last tile (of the tile before it where the last tile is that one pixel; S >= 2 and two tiles at least)."""
    rng = np.random.default_rng([shape[0], shape[1], S, 77])
    npix = shape[0] * shape[1]
    PHI = -np.abs(rng.standard_normal((npix, S))).astype(F32) - F32(0.25)
    owner = rng.integers(0, S + 1, npix)
    held = np.flatnonzero(owner < S)
    PHI[held, owner[held]] = 1 + owner[held]
    if S >= 2:
        twice = held[rng.random(held.size) < 0.1]
        PHI[twice, (owner[twice] + 1 + rng.integers(0, S - 1, twice.size)) % S] = F32(0.5)
    first, last = edges(shape)
    nan_at, negz_at, posz_at = specials(shape)
    PHI[nan_at, :] = -1
    PHI[nan_at, 0] = np.nan
    PHI[negz_at, :] = F32(-0.0)
    if posz_at != first:
        PHI[posz_at, :] = F32(0.0)
    PHI[last, :] = -1
    PHI[last, S - 1] = 3
    over = first if first != last else first - TILE
    if S >= 2 and over >= 0 and over != last:
        PHI[over, :] = -1
        PHI[over, 0] = PHI[over, S - 1] = 2
    return _frozen(PHI.reshape(shape[1], shape[0], S).transpose(1, 0, 2))[0]


# ---- values at the edge of the range ------------------------------------------------------------------------------------------------
# With cov = 1, t = dist/2: 1400, 1480 and 1500 give t = 700, 740 and 750, where exp(-t) is a small normal number, a float64
# subnormal, and 0.  1e-45 and 1e-38 are float32 subnormals; -1 and -Inf are no squared residuals, but nothing refuses them.
RANGE_DIST = tuple(F32(x) for x in (0.0, -0.0, 1e-45, 1e-38, 1e-8, 700.0, 1400.0, 1480.0, 1500.0, 3.4e38, np.inf, -1.0, -np.inf))
COV_EDGES = (5e-324, 1e-300, 1e-3, 1e300, np.inf, np.nan, 0.0, -1.0)
DH_EXACT = F32(0.02)
# What the recipe's dist is raised by in the range cases.  With all cov equal to 1 the c_s cancel and, where both likelihoods stand far
# above eps, DATA_s = (dist_r - dist_s)/2 but for rounding: a difference of two float32 numbers, which for two small dist is exactly
# half-way between two floats at about 1 pixel in 100.  There the last bit of exp decides the rounding to single, and "equal or
# adjacent on at most 1 in 1 000" cannot tell one correct maths library from another (the restatement against itself with exp one
# ulp off: 1.2 %).  From dist = 16 upwards (t >= 8, P <= 1.4e-4) eps's share of P + eps moves every such value off the half-way point
# by thousands of float64 ulps.  The small t of these cases are the laced ones; tests/test_segmentation_stage_cases.py asserts
# that a whole ulp in exp, expm1 or log now moves at most 1 DATA in 1 000.  The seam cases keep the recipe as it is: their cov differ.
BASE_DIST = F32(16.0)
STRIP = {"below": 0, "exact": 1, "above": 2}  # columns with no segment inside; DH = nextafter(0.02f, -1), 0.02f, nextafter(0.02f, +1)


def same_bits(a, b):
    return np.asarray(a, F32).view(np.uint32) == np.asarray(b, F32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def range_case(shape, S):
    """(PHI, dist, DH, together, alone): the recipe's random planes, dist raised by BASE_DIST; columns 0..2 hold no segment and have DH just below, at and
    just above 0.02f; each value of RANGE_DIST stands at one pixel in all segments at once, PHI alternating in sign over s (the
    memory positions `together`, one per value), and once per segment at a pixel of its own (`alone` [len(RANGE_DIST), S])."""
    rng = np.random.default_rng([shape[0], shape[1], S, 99])
    full = shape + (S,)
    PHI = rng.standard_normal(full).astype(F32)
    PHI[3, 5, 0] = np.nan
    PHI[4, 5, S - 1] = F32(-0.0)
    PHI[5, 5, 0] = F32(0.0)
    dist = ((rng.standard_normal(full) ** 2 * rng.choice([0.01, 1.0, 80.0], size=full)).astype(F32) + BASE_DIST).astype(F32)
    DH = (rng.random(full) * 0.05).astype(F32)
    PHI[:, :3, :] = -np.abs(PHI[:, :3, :]) - F32(0.1)
    DH[:, STRIP["below"], :] = np.nextafter(DH_EXACT, F32(-1))
    DH[:, STRIP["exact"], :] = DH_EXACT
    DH[:, STRIP["above"], :] = np.nextafter(DH_EXACT, F32(1))
    nv = len(RANGE_DIST)
    pool = rng.permutation(np.arange(6 * shape[0], shape[0] * shape[1]))  # clear of the strips and of PHI's NaN and zeros
    together = pool[:nv]
    alone = pool[nv:nv + nv * S].reshape(nv, S)
    for k, v in enumerate(RANGE_DIST):
        i, j = at(shape, together[k])
        dist[i, j, :] = v
        PHI[i, j, :] = np.where(np.arange(S) % 2 == 0, F32(1), F32(-1))
        for s in range(S):
            i, j = at(shape, alone[k, s])
            dist[i, j, s] = v
    return _frozen(PHI, dist, DH) + (together, alone)


def range_covs(S):
    """name -> cov [S]: all ones, and ones with one entry replaced by each of COV_EDGES in turn; at S = 17 all eight in one vector."""
    out = {"ones": np.ones(S)}
    if S >= 17:
        c = np.ones(S)
        c[1:17:2] = COV_EDGES
        out["all_edges"] = c
        return out
    for k, e in enumerate(COV_EDGES):
        c = np.ones(S)
        c[k % S] = e
        out["%g" % e] = c
    return out


RANGE_CASES = tuple((shape, S, name) for shape in RANGE_PLANES for S in STAGE_S for name in range_covs(S))


def range_id(c):
    return "%dx%dx%d-cov_%s" % (c[0][0], c[0][1], c[1], c[2])


# ---- the restatement's results, computed once -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def want_variance(shape, S, minCOV, cap, seed=0):
    PHI, dist, _ = seam_case(shape, S, seed)
    return sr.variance_in_order(PHI, dist, minCOV, cap)


@functools.lru_cache(maxsize=None)
def seam_cov(shape, S, seed=0):
    """The cov the data term of a seam case is given: the model's, floored at 1, cap 100 (always finite)."""
    return want_variance(shape, S, 1.0, 100.0, seed)[0]


@functools.lru_cache(maxsize=None)
def want_seam_data(shape, S, strategy, seed=0):
    PHI, dist, DH = seam_case(shape, S, seed)
    return sr.data_term(dist, PHI, DH, seam_cov(shape, S, seed), strategy)


@functools.lru_cache(maxsize=None)
def want_range_data(shape, S, name, strategy):
    PHI, dist, DH, _, _ = range_case(shape, S)
    return sr.data_term(dist, PHI, DH, range_covs(S)[name], strategy)
