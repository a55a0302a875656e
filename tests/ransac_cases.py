"""Inputs shared by tests/test_ransac_ref.py (CPU: the conditions on the fixtures) and tests/test_gpu_ransac.py (GPU: equality with
the restatement), and the mock-MEX build of mex/segmentation/SurfaceEquation.c.  Every case's restatement result is computed once
(functools.lru_cache) and never modified."""
import ctypes
import functools
import os
import subprocess

import numpy as np

import ransac_ref as ref

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG_DIR = os.path.join(ROOT, "pde-based-image-processing_amd", "mex", "segmentation")
MOCK_DIR = os.path.join(ROOT, "tests", "mexmock")
BUILD_DIR = os.path.join(MOCK_DIR, "_build")
TILE_SMALL = 256         # rows of a score tile below BIG_ROWS data rows (csrc/pdeip_ransac.hip)
BIG_ROWS = 32768         # from here on a score tile has TILE_BIG rows
TILE_BIG = 1024


def build_seg_stub(name, pdeip):
    """Compile mex/segmentation/<name>.c against the mock MEX runtime (tests/mexmock) and libpdeip.so."""
    os.makedirs(BUILD_DIR, exist_ok=True)
    so = os.path.join(BUILD_DIR, "segmentation_" + name + ".so")
    srcs = [os.path.join(SEG_DIR, name + ".c"), os.path.join(MOCK_DIR, "mexmock.c")]
    deps = srcs + [os.path.join(SEG_DIR, "..", "pdeip_mex_util.h"), os.path.join(MOCK_DIR, "mex.h"), pdeip.capi.LIB_PATH]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        libdir = os.path.dirname(pdeip.capi.LIB_PATH)
        subprocess.run(["gcc", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-shared", "-fPIC", "-I" + MOCK_DIR,
                        "-I" + os.path.join(ROOT, "include"), "-o", so] + srcs + ["-L" + libdir, "-lpdeip", "-Wl,-rpath," + libdir],
                       check=True)
    lib = ctypes.CDLL(so)
    lib.mock_make.restype = ctypes.c_void_p
    lib.mock_make.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_long), ctypes.c_int, ctypes.c_void_p]
    lib.mock_free.argtypes = [ctypes.c_void_p]
    lib.mock_data.restype = ctypes.c_void_p
    lib.mock_data.argtypes = [ctypes.c_void_p]
    lib.mock_ndim.argtypes = [ctypes.c_void_p]
    lib.mock_dim.restype = ctypes.c_long
    lib.mock_dim.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.mock_last_error.restype = ctypes.c_char_p
    lib.mock_call.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    return lib


# ---- data -------------------------------------------------------------------------------------------------------------------

PLANE = (0.031, -0.017, 12.5)                              # z = a*X + b*Y + c
QUADRIC = (2.0e-5, -1.5e-5, 1.0e-5, 0.012, 0.02, 20.0)     # z = a*X^2 + b*Y^2 + c*XY + d*X + e*Y + f


def surface_points(seed, ndata, order, noise=0.05, outliers=0.2, rows=480, cols=640):
    """A [ndata, ncoef], B [ndata] (single): pixels of a rows x cols grid on the surface PLANE / QUADRIC, Gaussian noise, and a
    fraction of outliers lifted by 3..15."""
    rng = np.random.default_rng(seed)
    X = rng.integers(1, cols + 1, ndata).astype(np.float64)
    Y = rng.integers(1, rows + 1, ndata).astype(np.float64)
    A = ref.design(X, Y, order)
    coef = np.array(PLANE if order == 1 else QUADRIC)
    z = A.astype(np.float64) @ coef + rng.normal(0, noise, ndata)
    out = rng.random(ndata) < outliers
    z[out] += rng.uniform(3, 15, ndata)[out] * rng.choice([-1, 1], ndata)[out]
    return np.asfortranarray(A), z.astype(F32)


def near_model(order, rel=1e-3):
    c = np.array(PLANE if order == 1 else QUADRIC)
    return (c * (1 + rel)).astype(F32)


# name -> dict(order, ndata, iter, given (bool), err_thr, min_set_size, seed)
MATRIX_CASES = {}


def _add(name, order, ndata, iter, given=False, err_thr=0.3, min_set_size=0.4, seed=1, data_seed=None):
    MATRIX_CASES[name] = dict(order=order, ndata=ndata, iter=iter, given=given, err_thr=err_thr, min_set_size=min_set_size, seed=seed,
                              data_seed=len(MATRIX_CASES) + 100 if data_seed is None else data_seed)


for _order in (1, 2):
    _n = 4 if _order == 1 else 7
    for _k, _nd in enumerate((_n, 63, 64, 65, TILE_SMALL - 1, TILE_SMALL, TILE_SMALL + 1)):
        _add("o%d_n%d" % (_order, _nd), _order, _nd, 2 if _k % 2 else 1, given=bool(_k % 3 == 1), seed=11 + _k)
_add("o1_n20011_i100_given", 1, 20011, 100, given=True, seed=5)
_add("o2_n20011_i100", 2, 20011, 100, seed=6)
_add("o1_big_below", 1, BIG_ROWS - 1, 2, seed=7)                       # the last size on 256-row tiles
_add("o2_big_at", 2, BIG_ROWS, 1, given=True, seed=8)                   # the first on 1024-row tiles, a whole number of them
_add("o1_big_tile_above", 1, BIG_ROWS + 1, 2, seed=9)                   # one row into the next 1024-row tile
_add("o2_big_odd", 2, BIG_ROWS + TILE_BIG - 1, 2, seed=10)              # one row below a 1024-row tile's end


@functools.lru_cache(maxsize=None)
def matrix_case(name):
    """(A, B, M_in or None, case dict, restatement result)."""
    c = MATRIX_CASES[name]
    A, B = surface_points(c["data_seed"], c["ndata"], c["order"])
    M_in = near_model(c["order"]) if c["given"] else None
    r = ref.surface_equation(A, B, M_in, c["err_thr"], c["min_set_size"], c["iter"], seed=c["seed"])
    for x in (A, B):
        x.setflags(write=False)
    return A, B, M_in, c, r


@functools.lru_cache(maxsize=None)
def explicit_sets_case():
    """300 points, order 1, five hypotheses given as a list: [1] is one index seven... four times (singular), [3] contains a row
    whose B is NaN."""
    A, B = surface_points(41, 300, 1)
    B = B.copy()
    B[17] = np.nan
    sets = ref.sample_sets(3, 5, 4, 300)
    sets[sets == 17] = 18
    sets[1, :] = 123
    sets[3, 2] = 17
    r = ref.surface_equation(A, B, None, 0.3, 0.4, 5, sets=sets)
    return A, B, sets, r


@functools.lru_cache(maxsize=None)
def best_inlier_tie_case():
    """min_set_size = 1.0 with outliers: no hypothesis is licit, the best-inlier path decides.  TIE_SEED makes the last of several
    hypotheses with the highest count differ in its bits from an earlier one: `>=` (the latest wins) shows in M_out."""
    A, B = surface_points(43, 65, 1, noise=0.2, outliers=0.3)
    r = ref.surface_equation(A, B, None, 0.3, 1.0, 12, seed=TIE_SEED)
    return A, B, r


TIE_SEED = 166


@functools.lru_cache(maxsize=None)
def given_wins_case():
    """No outliers, min_set_size = 1.0 and a threshold that takes every point: M_in is the float64 least-squares plane of all the
    points, so no licit hypothesis (one with every point as an inlier) has a smaller error sum."""
    A, B = surface_points(44, 300, 1, noise=0.05, outliers=0.0)
    M_in = np.linalg.lstsq(A.astype(np.float64), B.astype(np.float64), rcond=None)[0].astype(F32)
    r = ref.surface_equation(A, B, M_in, 1.0, 1.0, 20, seed=2)
    return A, B, M_in, r


def two_planes(nrows=64, ncols=80, seed=45, noise=0.01):
    """A [nrows x ncols] disparity: 70 % of the pixels on PLANE2000, 30 % on another plane (the outliers)."""
    rng = np.random.default_rng(seed)
    jj, ii = np.meshgrid(np.arange(ncols) + 1.0, np.arange(nrows) + 1.0)
    D = PLANE2000[0] * jj + PLANE2000[1] * ii + PLANE2000[2] + rng.normal(0, noise, (nrows, ncols))
    other = rng.random((nrows, ncols)) < 0.3
    D[other] = (-0.02 * jj + 0.04 * ii + 30.0 + rng.normal(0, noise, (nrows, ncols)))[other]
    return np.asfortranarray(D.astype(F32))


PLANE2000 = (0.05, 0.02, 8.0)


@functools.lru_cache(maxsize=None)
def iter2000_case():
    D = two_planes()
    A, B = ref.masked_data(np.ones_like(D), D, 1)
    r = ref.surface_equation(A, B, None, 0.1, 0.5, 2000, seed=2000)
    return np.asfortranarray(A), B, r


# ---- the masked form ----------------------------------------------------------------------------------------------------------

def masks(nrows, ncols):
    ii, jj = np.meshgrid(np.arange(nrows), np.arange(ncols), indexing="ij")
    rng = np.random.default_rng(nrows * 1000 + ncols)
    laced = rng.uniform(-1, 1, (nrows, ncols))
    laced[rng.random((nrows, ncols)) < 0.2] = np.nan
    blob = 0.3 * min(nrows, ncols) - np.hypot(ii - 0.45 * nrows, jj - 0.55 * ncols)
    col = -np.ones((nrows, ncols))
    col[:, ncols // 3] = 0.0  # PHI == 0 counts
    col[0, ncols // 3] = -0.0
    return {"all": np.ones((nrows, ncols)), "none": -np.ones((nrows, ncols)), "column": col,
            "checker": np.where((ii + jj) % 2 == 0, 1.0, -1.0), "nan_laced": laced, "blob": blob}


# name -> (nrows, ncols, mask name, order, iter, given, seed)
MASKED_CASES = {}
for _k, _m in enumerate(("all", "none", "column", "checker", "nan_laced", "blob")):
    for _order in (1, 2):
        MASKED_CASES["%s_o%d" % (_m, _order)] = (37, 53, _m, _order, 20, bool((_k + _order) % 2), 60 + _k)
MASKED_CASES["checker_big_o1"] = (200, 170, "checker", 1, 6, False, 70)  # 34000 pixels: 1024-row tiles, 17000 data rows
MASKED_CASES["none_nogiven_o2"] = (37, 53, "none", 2, 20, False, 71)


@functools.lru_cache(maxsize=None)
def masked_case(name):
    """(PHI, D, order, M_in, iter, seed, restatement tuple of ransac_ref.surface_fit_masked)."""
    nrows, ncols, m, order, iter, given, seed = MASKED_CASES[name]
    PHI = np.asfortranarray(masks(nrows, ncols)[m].astype(F32))
    D = two_planes(nrows, ncols, seed=seed, noise=0.02)
    M_in = np.array(PLANE2000 if order == 1 else (0, 0, 0) + PLANE2000, F32) * F32(1.001) if given else None
    want = ref.surface_fit_masked(PHI, D, order, M_in, 0.1, 0.3, iter, seed=seed)
    return PHI, D, order, M_in, iter, seed, want


def all_margins():
    """[(case name, margins of the restatement's scan, models, given model)] of every input the GPU tests run."""
    out = []
    for name in MATRIX_CASES:
        _, _, M_in, _, r = matrix_case(name)
        out.append((name, r, M_in))
    out.append(("explicit_sets", explicit_sets_case()[3], None))
    out.append(("best_inlier_tie", best_inlier_tie_case()[2], None))
    out.append(("given_wins", given_wins_case()[3], given_wins_case()[2]))
    out.append(("iter2000", iter2000_case()[2], None))
    for name in MASKED_CASES:
        c = masked_case(name)
        if c[6][0] is not None:
            out.append(("masked_" + name, c[6][0], c[3]))
    return out
