"""Fixtures of the sparse driver's tests (tests/test_sparse_ref.py on the CPU, tests/test_gpu_sparse.py on the GPU).  Everything is
generated from fixed seeds; the restatement's runs (sparse_ref.py) are computed once per process and shared.

Filter cases (FILTER_CASES: name -> float32 plane): what tests/test_sparse_ref.py::test_filter_cases_hold_what_they_claim asserts.
  nan_counts_interior    ten 5x5 blocks side by side: the centre window of block c holds exactly c NaNs (0..9), the rest distinct values
  nan_counts_edge        the same on the top edge (0..6 NaNs among the six in-plane positions: the three zeros of the padding decide)
  corner_nan0 .. 4       4x4 planes with 0..4 NaNs among the four in-plane positions of the corner's window (five zeros)
  even_inexact           interior windows with 2, 4, 6 and 8 numbers whose two middle values are neighbouring floats: the mean lies
                         half-way between two float32 values and must be rounded to even
  inf_pairs              windows of two / four numbers with (-Inf, +Inf), (+Inf, +Inf), (-Inf, -Inf) in the middle
  plateaus               a constant plane and a plane of the integers 0..2 (ties everywhere)
  both_zeros             -0 and +0 mixed with a few NaNs and values
  all_nan                every pixel NaN: the interior stays NaN, the border (which sees the padding's zeros) becomes 0

Driver fixtures, all 60x80: three_planes (cropped, see below) with 15 % random NaNs plus one 7x8 NaN block; scl_factor 0.75 and pyr_scl 0.55 give K = 3
(60x80, 45x60, 34x45).  Consensus sizes are 1.1 .. 1.7 for the reason given in seeds_cases.py (no hypothesis reaches the consensus
size, so no `sum < best` comparison is made); sp_short_cset keeps the driver's 0.1, 0.16, 0.22.  The seeds were searched so that the
restatement alone meets the conditions tests/test_sparse_ref.py asserts.
  The block's place.  After nanmedfilt2 the block's 5x6 core stays NaN, nan_fill makes it an outlier of every surface, and over the
drivers' 20 iterations PHI saturates to -5 inside it and +5 around it: a sharp edge along the core.  Shrinking 60 -> 45 rows puts the
centre of every third output row exactly on an input row boundary (between the 0-based rows 4m+1 and 4m+2), where the cubic
weights of a +5 / -5 step cancel to rounding noise (1e-17): a `>= 0` decision on a knife's edge.  The block therefore starts at row
26 and column 50, so that none of its core's four edges (26|27, 31|32, 50|51, 56|57) is such a boundary.
For the same reason the map is the first 60 rows of a 64x80 three_planes scene: the two right-hand planes then meet between rows
31 and 32, where a 60-row scene would have them meet between rows 29 and 30, one of those boundaries.

DRIFT[case]: as in seeds_cases.py -- the largest |PHI| difference over all iterations between the restatement and its run with DATA
moved by one ulp on a seeded 1 % of the pixels, every decision identical.  Measured by
    python -m pytest tests/test_sparse_ref.py -q -s -k drift
which prints the values and asserts that the ones recorded here are what it measures (not below, at most twice above).
"""
import functools

import numpy as np

import seeds_cases as sc
import segmentation_ref as sr
import sparse_ref as sp

F32 = np.float32
NAN = F32(np.nan)
PERTURB_SEED = sc.PERTURB_SEED
CSET = sc.CSET
CSET_DRIVER = sc.CSET_DRIVER
SCL, PYR = 0.75, 0.55
WINDOW = [(di, dj) for dj in (-1, 0, 1) for di in (-1, 0, 1)]


# ---- filter cases --------------------------------------------------------------------------------------------------------------

def _distinct(shape, rng):
    n = int(np.prod(shape))
    return (rng.permutation(n).astype(F32) * F32(0.37) - F32(3.0)).reshape(shape)


def _nan_counts_interior():
    rng = np.random.default_rng(101)
    A = _distinct((5, 50), rng)
    for c in range(10):
        for k in rng.permutation(9)[:c]:
            A[2 + WINDOW[k][0], 5 * c + 2 + WINDOW[k][1]] = NAN
    return A


def _nan_counts_edge():
    rng = np.random.default_rng(102)
    A = _distinct((5, 35), rng)
    inplane = [(di, dj) for di, dj in WINDOW if di >= 0]
    for c in range(7):
        for k in rng.permutation(6)[:c]:
            A[0 + inplane[k][0], 5 * c + 2 + inplane[k][1]] = NAN
    return A


def _corner(c):
    rng = np.random.default_rng(110 + c)
    A = _distinct((4, 4), rng) + F32(5.0)  # positive: the padding's zeros are the smallest values of the window
    inplane = [(0, 0), (1, 0), (0, 1), (1, 1)]
    for k in rng.permutation(4)[:c]:
        A[inplane[k]] = NAN
    return A


def _even_inexact():
    """Block e (n = 2, 4, 6, 8 numbers): below the middle n/2 - 1 small values, the middle pair (m, nextafter(m)), above it n/2 - 1
    large ones, 9 - n NaNs, in a seeded order."""
    rng = np.random.default_rng(103)
    A = np.full((5, 20), F32(-50.0))
    for e, n in enumerate((2, 4, 6, 8)):
        m = F32(1.0) + F32(e) * F32(0.7)
        vals = [m, np.nextafter(m, F32(np.inf))] + [F32(-10 - k) for k in range(n // 2 - 1)] + [F32(10 + k) for k in range(n // 2 - 1)]
        vals += [NAN] * (9 - n)
        for k, pos in enumerate(rng.permutation(9)):
            A[2 + WINDOW[pos][0], 5 * e + 2 + WINDOW[pos][1]] = vals[k]
    return A


def _inf_pairs():
    inf = F32(np.inf)
    A = np.full((5, 20), NAN)
    for e, vals in enumerate(([-inf, inf], [inf, inf], [-inf, -inf], [-inf, -inf, inf, inf])):
        for k, v in enumerate(vals):
            A[2 + WINDOW[2 * k][0], 5 * e + 2 + WINDOW[2 * k][1]] = v
    return A


def _both_zeros():
    rng = np.random.default_rng(104)
    A = np.where(rng.random((9, 11)) < 0.5, F32(-0.0), F32(0.0)).astype(F32)
    A[rng.random(A.shape) < 0.15] = NAN
    A[rng.random(A.shape) < 0.15] = F32(2.5)
    A[rng.random(A.shape) < 0.10] = F32(-1.5)
    return A


@functools.lru_cache(maxsize=None)
def filter_cases():
    rng = np.random.default_rng(105)
    cases = {
        "nan_counts_interior": _nan_counts_interior(),
        "nan_counts_edge": _nan_counts_edge(),
        "even_inexact": _even_inexact(),
        "inf_pairs": _inf_pairs(),
        "plateau_constant": np.full((6, 9), F32(7.0)),
        "plateau_ties": rng.integers(0, 3, (17, 13)).astype(F32),
        "both_zeros": _both_zeros(),
        "all_nan": np.full((6, 7), NAN),
    }
    for c in range(5):
        cases["corner_nan%d" % c] = _corner(c)
    return {k: np.asfortranarray(v.astype(F32)) for k, v in cases.items()}


FILTER_NAMES = ["all_nan", "both_zeros", "corner_nan0", "corner_nan1", "corner_nan2", "corner_nan3", "corner_nan4", "even_inexact", "inf_pairs",
                "nan_counts_edge", "nan_counts_interior", "plateau_constant", "plateau_ties"]
# (rows, cols, frames): degenerate planes, wave seams (63 / 64 / 65 rows), workgroup seams (255 / 256 / 257 rows), the frame stride
RANDOM_SHAPES = [(1, 1, 1), (1, 7, 1), (7, 1, 1), (2, 2, 1), (3, 3, 1), (63, 4, 1), (64, 4, 1), (65, 4, 1), (255, 5, 1), (256, 5, 1), (257, 5, 1),
                 (300, 7, 3)]
NAN_SHARES = (0.0, 0.3, 0.9)


def random_plane(shape, share, seed=7):
    rows, cols, frames = shape
    rng = np.random.default_rng([seed, rows, cols, frames, int(share * 100)])
    A = (rng.standard_normal((rows, cols, frames)) * 4.0).astype(F32)
    A[rng.random(A.shape) < share] = NAN
    return np.asfortranarray(A if frames > 1 else A[:, :, 0])


# ---- driver fixtures ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def sparse_map(seed=21):
    """three_planes at 60x80 (the first 60 rows of a 64x80 scene) with 15 % random NaNs and one 7x8 NaN block."""
    D = sc.three_planes(64, 80, seed)[0][:60].copy()
    rng = np.random.default_rng(seed + 1000)
    D[rng.random(D.shape) < 0.15] = NAN
    D[26:33, 50:58] = NAN  # rows 26..32: see "The block's place" above
    D = np.asfortranarray(D)
    D.setflags(write=False)
    return D


def _band():
    AA = np.ones((60, 80), F32)
    AA[:, 30:44] = 0
    return AA


def _tiny():
    AA = np.zeros((60, 80), F32)
    AA[20:24, 30:34] = 1
    return AA


def _given_phi():
    P = -np.ones((60, 80, 2), F32)
    P[6:54, 4:28, 0] = 1
    P[4:26, 40:76, 1] = 1
    return np.asfortranarray(P)


def _seeds_case(order=1, sigmaLim=0.7, cset=CSET, iterations=8, AA=None, seeds=3, seed=11):
    return dict(D=sparse_map(), order=order, sigmaLim=sigmaLim, cset_vect=list(cset), iterations=iterations, AA=AA, seeds=seeds, scl_factor=SCL,
                pyr_scl=PYR, seed=seed)


SEEDS_CASES = {
    "sp_seeds_o1": lambda: _seeds_case(order=1, seed=1),
    "sp_seeds_o2": lambda: _seeds_case(order=2, seed=12),
    "sp_band": lambda: _seeds_case(order=2, AA=_band(), seed=3),
    "sp_tiny_aa": lambda: _seeds_case(order=2, AA=_tiny()),
    "sp_short_cset": lambda: _seeds_case(order=2, cset=CSET_DRIVER[:3], iterations=4, seeds=1, seed=2),
}
RC_CASES = {
    "sp_rc": lambda: dict(D=sparse_map(), PHI=_given_phi(), order=2, strategy=sr.INVERSE, sigmaLim=1.0, ransac_cset=F32(1.7), iterations=6,
                          srem_thr=0.002, scl_factor=SCL, rc_scl=PYR, seed=4),
}
_DRV = dict(ransac_min_cset=1.1, ransac_max_cset=1.7)
DRIVER_CASES = {
    "sp_driver_seeds1": lambda: dict(Din=sparse_map(), PHI=None, seed=1, seeds=1, **_DRV),
    "sp_driver_seeds3": lambda: dict(Din=sparse_map(), PHI=None, seed=2, seeds=3, polyorder=1, **_DRV),
    "sp_driver_phi_given": lambda: dict(Din=sparse_map(), PHI=_given_phi(), seed=4, **_DRV),
}
ALL = sorted(SEEDS_CASES) + sorted(RC_CASES) + sorted(DRIVER_CASES)
DRIFT = {"sp_seeds_o1": 1.4e-5, "sp_seeds_o2": 1.1e-5, "sp_band": 1.7e-5, "sp_tiny_aa": 0.0, "sp_short_cset": 2.2e-6, "sp_rc": 2.2e-6,
         "sp_driver_seeds1": 3.8e-6, "sp_driver_seeds3": 1.9e-5, "sp_driver_phi_given": 4.9e-6}


def _run(name, perturb, trace, **over):
    if name in SEEDS_CASES:
        a = SEEDS_CASES[name]()
        a.update(over)
        D = a.pop("D")
        return sp.generate_seeds(D, a.pop("order"), a.pop("sigmaLim"), a.pop("cset_vect"), a.pop("iterations"), perturb=perturb, trace=trace, **a)
    if name in RC_CASES:
        a = RC_CASES[name]()
        a.update(over)
        return sp.region_competition(a.pop("D"), a.pop("PHI"), a.pop("order"), a.pop("strategy"), a.pop("sigmaLim"), a.pop("ransac_cset"),
                                     a.pop("iterations"), a.pop("srem_thr"), perturb=perturb, trace=trace, **a)
    a = DRIVER_CASES[name]()
    a.update(over)
    return sp.disp_segmentation_sparse(a.pop("Din"), perturb=perturb, trace=trace, **a)


@functools.lru_cache(maxsize=None)
def run(name, perturbed=False):
    """The restatement's run of a case: (result dict, trace).  Computed once and shared; callers must not modify it."""
    trace = []
    return _run(name, sr.make_perturb(PERTURB_SEED) if perturbed else None, trace), trace


def run_variant(name, **over):
    """The case with arguments replaced (pyramid=..., gamma0=...): (result dict, trace).  Not cached."""
    trace = []
    return _run(name, None, trace, **over), trace
