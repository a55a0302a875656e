"""Inputs of the region-competition tests (tests/test_segmentation_ref.py on the CPU, tests/test_gpu_segmentation.py on the GPU).
Everything is generated from fixed seeds; the restatement's results are computed once per process and shared.

End-to-end cases (END_TO_END): name -> the arguments of segmentation_ref.level / region_competition.
  dense48x64   a 48x64 disparity map of two planes (left / right of column 32) plus a quadratic patch, noise sigma 0.05; four
               box-shaped segments PHI = +-1: one per plane, one of 5 pixels (removed at iteration 1) and one on the patch,
               which no plane fits: it shrinks and drops under srem_thr at iteration 4, an EVEN one (test_segmentation_ref
               asserts both)
  sparse37x53  a 37x53 map (no side a multiple of 64 or of the 256-pixel tile) of two planes with NaNs, the sparse driver's form:
               nan_fill 1000 puts dist values on both sides of dist_cap = 100
  rc60x80      60x80, three segments, scl_factor 0.7 and rc_scl 0.4 (three scales, six visits), 6 iterations per visit

DRIFT[case]: the largest |PHI| difference over all iterations between the restatement and its run with DATA moved by one single
ulp on a seeded 1 % of the pixels (segmentation_ref.make_perturb(PERTURB_SEED)), masks and surfaces staying identical.  Measured
on the CPU by
    python -m pytest tests/test_segmentation_ref.py -q -s -k drift
which prints the values and asserts that the ones recorded here are what it measures (not below, at most twice above).
"""
import functools

import numpy as np

import segmentation_ref as sr

F32 = np.float32
PERTURB_SEED = 20240611
DRIFT = {"dense48x64": 1.5e-6, "sparse37x53": 1.5e-6, "rc60x80": 2.4e-6}


def _box(shape, r0, r1, c0, c1):
    P = -np.ones(shape, F32)
    P[r0:r1, c0:c1] = 1
    return P


def two_planes(nrows, ncols, seed, split=None, patch=None, sigma=0.05):
    """(D float32, truth int: 1 left plane, 2 right plane, 0 the quadratic patch)."""
    rng = np.random.default_rng(seed)
    split = ncols // 2 if split is None else split
    y, x = np.mgrid[1:nrows + 1, 1:ncols + 1].astype(np.float64)
    left = 10.0 + 0.05 * x + 0.02 * y
    right = 20.0 - 0.03 * x + 0.04 * y
    D = np.where(x <= split, left, right)
    truth = np.where(x <= split, 1, 2)
    if patch is not None:
        r0, r1, c0, c1 = patch
        q = 30.0 + 0.15 * (x - 0.5 * (c0 + c1)) ** 2 + 0.15 * (y - 0.5 * (r0 + r1)) ** 2
        D[r0:r1, c0:c1] = q[r0:r1, c0:c1]
        truth[r0:r1, c0:c1] = 0
    D = D + sigma * rng.standard_normal(D.shape)
    return np.asfortranarray(D.astype(F32)), truth


@functools.lru_cache(maxsize=None)
def dense48x64():
    D, truth = two_planes(48, 64, 29, patch=(30, 48, 24, 40))
    shape = D.shape
    PHI = np.stack([_box(shape, 6, 42, 5, 27), _box(shape, 6, 42, 37, 59), _box(shape, 2, 3, 50, 55), _box(shape, 34, 44, 27, 37)], axis=2)
    args = dict(order=1, strategy=sr.INVERSE, minCOV=1.0, ransac_cset=0.7, iterations=20, srem_thr=0.0314, seed=7, prm=dict(sr.DENSE))
    return D, np.asfortranarray(PHI), truth, args


@functools.lru_cache(maxsize=None)
def sparse37x53():
    D, truth = two_planes(37, 53, 12, split=26)
    rng = np.random.default_rng(13)
    D = D.copy()
    D[rng.random(D.shape) < 0.06] = np.nan
    shape = D.shape
    PHI = np.stack([_box(shape, 6, 30, 3, 22), _box(shape, 6, 30, 31, 50)], axis=2)
    args = dict(order=1, strategy=sr.INVERSE, minCOV=1.2, ransac_cset=0.5, iterations=12, srem_thr=0.01, seed=3, prm=dict(sr.SPARSE))
    return np.asfortranarray(D), np.asfortranarray(PHI), truth, args


@functools.lru_cache(maxsize=None)
def rc60x80():
    D, truth = two_planes(60, 80, 14, patch=(40, 56, 30, 50))
    shape = D.shape
    PHI = np.stack([_box(shape, 10, 40, 5, 32), _box(shape, 10, 40, 48, 76), _box(shape, 42, 54, 32, 48)], axis=2)
    args = dict(order=2, strategy=sr.INVERSE, sigmaLim=1.5, ransac_cset=0.6, iterations=6, srem_thr=0.002, scl_factor=0.7, rc_scl=0.4, seed=5,
                prm=dict(sr.DENSE))
    return D, np.asfortranarray(PHI), truth, args


END_TO_END = {"dense48x64": dense48x64, "sparse37x53": sparse37x53, "rc60x80": rc60x80}


@functools.lru_cache(maxsize=None)
def run(name, perturbed=False):
    """The restatement's run of an end-to-end case: (result dict, trace).  Computed once and shared; callers must not modify it."""
    D, PHI, _, args = END_TO_END[name]()
    trace = []
    perturb = sr.make_perturb(PERTURB_SEED) if perturbed else None
    fn = sr.region_competition if name == "rc60x80" else sr.level
    return fn(PHI=PHI, D=D, perturb=perturb, trace=trace, **args), trace


STAGE_SHAPES = ((37, 53), (48, 64))
STAGE_S = (1, 2, 3, 17)


@functools.lru_cache(maxsize=None)
def stage_case(shape, S, seed=0, nan_dist=False):
    """Random planes for the stage kernels: PHI with a NaN and a -0.0, dist = a squared residual with values on both sides of 100
    (and a NaN when asked), DH on both sides of 0.02."""
    rng = np.random.default_rng(1000 * S + shape[0] + seed)
    PHI = rng.standard_normal(shape + (S,)).astype(F32)
    PHI[3, 5, 0] = np.nan
    PHI[4, 5, S - 1] = F32(-0.0)
    PHI[5, 5, 0] = F32(0.0)
    dist = (rng.standard_normal(shape + (S,)) ** 2 * rng.choice([0.01, 1.0, 80.0], size=shape + (S,))).astype(F32)
    dist[0, 0, :] = 0  # t = 0: where the .m's c - P cancels completely
    if nan_dist:
        dist[7, 9, S - 1] = np.nan
        PHI[7, 9, S - 1] = 1
    DH = (rng.random(shape + (S,)) * 0.05).astype(F32)
    return np.asfortranarray(PHI), np.asfortranarray(dist), np.asfortranarray(DH)
