"""Fixtures of the generateSeeds() / DispSegmentation tests (tests/test_seeds_ref.py on the CPU, tests/test_gpu_seeds.py on the
GPU).  Everything is generated from fixed seeds (chosen so that the restatement alone meets the
conditions test_seeds_ref.py asserts); the restatement's runs are computed once per process and shared.

  planes60x80_o1 / _o2   60x80, three noisy planar regions, scl_factor 0.7, pyr_scl 0.4 (K = 3: 60x80, 42x56, 30x40), 4 seeds, 8
                         iterations, orders 1 and 2
  sparse37x53            37x53 with NaN holes and the sparse constants (dist_cap 100, nan_fill 1000, mincov_gate 0.5)
  band60x80              an AA that excludes a band of columns
  tiny_aa                an AA of 4x4 allowed pixels: every seed is EMPTY at once, S = 0, gamma shrinks
  used_up                an AA of one block that the first seed fills: the later seeds find the allowed area used up
  short_cset / _o2       cset_vect shorter than iterations, the driver's own first entries (see below), orders 1 and 2
  zero_iterations        iterations = 0, scl_factor 0.3 (60x80, 18x24): the seed grid resized is negative everywhere, so v = K finds no
                         foreground (the grid at 0.7 would be dozens of components of equal area: a tie)
  driver_*               the dense driver at 60x80: param.PHI empty with seeds = 1 and seeds = 3, param.PHI given

Consensus sizes.  With the driver's cset_vect (0.1 .. 0.7) a 60x80 run of 4 seeds makes some 15 000 `sum < best` comparisons between
RANSAC hypotheses, of which about ten fall within 1e-3 relative whatever the seed (measured minima over runs: 3e-5 .. 3e-4), so no
seed gives a fixture whose every comparison clears 1e-3.  The fixtures therefore use cset_vect = 1.1 .. 1.7 (and the driver cases
ransac_min_cset / ransac_max_cset likewise): no hypothesis reaches the consensus size, every fit is decided by the exact integer
inlier counts, and no sum comparison is made at all.  short_cset and short_cset_o2 keep the driver's first entries (0.1, 0.16, 0.22) with one
seed and 4 iterations -- few enough comparisons for a seed to exist whose smallest margin exceeds 1e-3 (test_seeds_ref prints it).

DRIFT[case]: the largest |PHI| difference over all iterations between the restatement and its run with DATA moved by one single
ulp on a seeded 1 % of the pixels (segmentation_ref.make_perturb(PERTURB_SEED)), every decision staying identical.  Measured on the
CPU by
    python -m pytest tests/test_seeds_ref.py -q -s -k drift
which prints the values and asserts that the ones recorded here are what it measures (not below, at most twice above).
"""
import functools

import numpy as np

import seeds_ref as gs
import segmentation_ref as sr

F32 = np.float32
PERTURB_SEED = 20240611
CSET = gs.cset_vector(1.1, 1.7, 10)  # see above: no hypothesis reaches the consensus size
CSET_DRIVER = gs.cset_vector(0.1, 0.7, 10)


def three_planes(nrows, ncols, seed, sigma=0.05):
    """(D float32, truth int 1..3): left third, right upper and right lower regions, each a plane."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[1:nrows + 1, 1:ncols + 1].astype(np.float64)
    a = 10.0 + 0.05 * x + 0.02 * y
    b = 22.0 - 0.03 * x + 0.04 * y
    c = 34.0 + 0.02 * x - 0.05 * y
    truth = np.where(x <= ncols * 0.4, 1, np.where(y <= nrows * 0.5, 2, 3))
    D = np.where(truth == 1, a, np.where(truth == 2, b, c)) + sigma * rng.standard_normal(a.shape)
    return np.asfortranarray(D.astype(F32)), truth


def _seeds_case(D, order=1, sigmaLim=0.7, cset=CSET, iterations=8, AA=None, seeds=4, scl_factor=0.7, pyr_scl=0.4, seed=11, prm=None):
    return dict(D=D, order=order, sigmaLim=sigmaLim, cset_vect=list(cset), iterations=iterations, AA=AA, seeds=seeds, scl_factor=scl_factor,
                pyr_scl=pyr_scl, seed=seed, prm=dict(prm or gs.DENSE))


def _d60():
    return three_planes(60, 80, 21)[0]


def _sparse():
    D = three_planes(37, 53, 22)[0].copy()
    rng = np.random.default_rng(23)
    D[rng.random(D.shape) < 0.004] = np.nan  # a handful of holes: each spreads over 4x4 pixels per cubic resize
    return np.asfortranarray(D)


def _band():
    AA = np.ones((60, 80), F32)
    AA[:, 30:44] = 0
    return AA


def _block(r0, r1, c0, c1):
    AA = np.zeros((60, 80), F32)
    AA[r0:r1, c0:c1] = 1
    return AA


SEEDS_CASES = {
    "planes60x80_o1": lambda: _seeds_case(_d60(), order=1, seed=435562),
    "planes60x80_o2": lambda: _seeds_case(_d60(), order=2, seed=134640),
    "sparse37x53": lambda: _seeds_case(_sparse(), prm=gs.SPARSE, seeds=3, seed=277182),
    "band60x80": lambda: _seeds_case(_d60(), AA=_band(), seeds=3, seed=7),
    "tiny_aa": lambda: _seeds_case(_d60(), AA=_block(20, 24, 30, 34), seeds=3),
    "used_up": lambda: _seeds_case(_d60(), AA=_block(4, 28, 4, 28), seeds=3, seed=9),
    "short_cset": lambda: _seeds_case(_d60(), cset=CSET_DRIVER[:3], iterations=4, seeds=1, seed=3),
    "short_cset_o2": lambda: _seeds_case(_d60(), order=2, cset=CSET_DRIVER[:3], iterations=4, seeds=1, seed=23774),
    "zero_iterations": lambda: _seeds_case(_d60(), iterations=0, seeds=2, scl_factor=0.3, pyr_scl=0.2),
}
DRIVER_CASES = {
    "driver_seeds1": lambda: dict(Din=_d60(), PHI=None, seed=3, seeds=1, rc_scl=0.4, gen_scl=0.4, ransac_min_cset=1.1, ransac_max_cset=1.7),
    "driver_seeds3": lambda: dict(Din=_d60(), PHI=None, seed=372210, seeds=3, rc_scl=0.4, gen_scl=0.4, ransac_min_cset=1.1, ransac_max_cset=1.7),
    "driver_phi_given": lambda: dict(Din=_d60(), PHI=_given_phi(), seed=395967, rc_scl=0.4, gen_scl=0.4, ransac_min_cset=1.1, ransac_max_cset=1.7),
}
DRIFT = {"planes60x80_o1": 5.4e-6, "planes60x80_o2": 4.6e-6, "sparse37x53": 2.5e-5, "band60x80": 1.6e-5, "tiny_aa": 0.0, "used_up": 2.1e-6,
         "short_cset": 2.6e-6, "short_cset_o2": 2.1e-6, "zero_iterations": 0.0, "driver_seeds1": 5.1e-6, "driver_seeds3": 2.1e-5, "driver_phi_given": 1.9e-5}


def _given_phi():
    P = -np.ones((60, 80, 2), F32)
    P[6:54, 4:28, 0] = 1
    P[4:26, 40:76, 1] = 1
    return np.asfortranarray(P)


@functools.lru_cache(maxsize=None)
def run(name, perturbed=False):
    """The restatement's run of a case: (result dict, trace).  Computed once and shared; callers must not modify it."""
    trace = []
    perturb = sr.make_perturb(PERTURB_SEED) if perturbed else None
    if name in SEEDS_CASES:
        a = SEEDS_CASES[name]()
        D = a.pop("D")
        return gs.generate_seeds(D, a.pop("order"), a.pop("sigmaLim"), a.pop("cset_vect"), a.pop("iterations"), perturb=perturb, trace=trace,
                                 **a), trace
    a = DRIVER_CASES[name]()
    return gs.disp_segmentation(a.pop("Din"), perturb=perturb, trace=trace, **a), trace
