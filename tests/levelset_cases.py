"""The inputs of the level-set edge tests (tests/test_gpu_gac_stages.py, tests/test_gpu_line_edges.py), each chosen for one way a
kernel of csrc/pdeip_levelset.hpp, pdeip_cv.hpp or pdeip_diffusion.hpp can go wrong, and the functions that say what a case contains.
tests/test_levelset_cases.py proves on the CPU that every case is what its name says; without that a case could pass while testing
nothing.  Arrays are MATLAB-shaped float32 [rows, cols(, F)], built once per process and read-only; references are computed once per
process and shared (levelset_ref.py, cv_ref.py, diffusion_ref.py).

Selection (k_sel_init / k_sel_hist / k_sel_pick).  A case is a vector x, a 1-based rank k and a kind:
    sensitive   both neighbours of the k-th sorted value differ from it (where they exist): a rank off by one either way is seen
    edge        exactly one neighbour differs: the rank sits on the last / first element of a plateau
    tied        both neighbours equal it: only a rank that leaves the plateau is seen
The kind is part of the case's name.  np.sort is the reference: NaN last, as MATLAB's sort.  The kernel's key puts -0.0 below +0.0
while np.sort (and MATLAB's) leaves zeros in the order they came, so where the selected element is a zero of a plateau that mixes
both signs, only its VALUE is defined: those cases carry zero=True and are compared by value, as the median test of
test_gpu_stage_edges.py does.  k_sel_hist runs 256 lanes on at most 1024 workgroups: n = 262 144 is the last size of one trip.

The rank of the drivers is MATLAB's round(0.7*N) on the double product, which is not (7N+5)/10: 0.7*45 is 31.499999999999996.
"""
import functools

import numpy as np

import cv_ref
import diffusion_ref
import levelset_ref as ref

F32 = np.float32
HIST_SPAN = 1024 * 256  # elements one trip of k_sel_hist's grid-stride loop covers


def _ro(a, order="F"):
    a = np.asfortranarray(a, dtype=F32) if order == "F" else np.ascontiguousarray(a, dtype=F32)
    a.setflags(write=False)
    return a


def same(a, b):
    """Equal as the bitwise comparison sees two scalars: same bits, or both NaN."""
    a, b = F32(a), F32(b)
    return bool((np.isnan(a) and np.isnan(b)) or a.view(np.uint32) == b.view(np.uint32))


# ---- selection -----------------------------------------------------------------------------------------------------------------

def driver_rank(n):
    """round(0.7*N) as the driver and MATLAB take it: the double product, rounded half away from zero; at least 1."""
    return max(int(np.floor(0.7 * float(n) + 0.5)), 1)


def exact_rank(n):
    """(7N+5)/10 in integers: what a tidy-up of driver_rank would compute, and not what MATLAB does."""
    return (7 * n + 5) // 10


SEL_SIZES = (1, 2, 255, 256, 257, HIST_SPAN - 1, HIST_SPAN, HIST_SPAN + 1, HIST_SPAN + 257)
ROUND_N = (45, 85, 165)  # the first N where driver_rank and exact_rank part (with 175, 325, ...)


def _distinct(n, seed):
    """n distinct values of both signs around an exact zero, in random order."""
    rng = np.random.default_rng([seed, n])
    return ((rng.permutation(n).astype(np.int64) - n // 3).astype(F32) * F32(0.37)).astype(F32)


def sel_kind(x, k):
    """sensitive / edge / tied, read off the sorted data; the zeros of a mixed plateau count as equal (their order is not defined)."""
    Y = np.sort(np.asarray(x, F32).ravel())
    me = Y[k - 1]

    def eq(v):
        return same(v, me) or (v == 0 and me == 0)

    nb = [Y[j] for j in (k - 2, k) if 0 <= j < Y.size]
    n_eq = sum(1 for v in nb if eq(v))
    if n_eq == 0:
        return "sensitive"
    return "tied" if n_eq == len(nb) else "edge"


def _sel_table():
    T = {}

    def add(name, x, k, zero=False):
        x = np.asarray(x, F32)
        full = "%s_%s" % (name, sel_kind(x, k))
        assert full not in T, full
        T[full] = (_ro(x, "C"), int(k), zero)

    for n in SEL_SIZES:
        x = _distinct(n, 1)
        for what, k in (("first", 1), ("last", n), ("r70", driver_rank(n))):
            if n <= 2 and what == "r70":
                continue  # round(0.7) = 1 and round(1.4) = 1: the "first" case
            add("n%d_%s" % (n, what), x, k)
    for n in ROUND_N:
        add("round_n%d" % n, _distinct(n, 2), driver_rank(n))
    n, rng = 777, np.random.default_rng(3)
    add("all_equal", np.full(n, 0.3, F32), 400)
    two = rng.permutation(np.r_[np.full(500, 0.25, F32), np.full(n - 500, 0.5, F32)])
    add("two_values_last_of_lower", two, 500)
    add("two_values_first_of_upper", two, 501)
    # negative, positive and subnormal values of both signs, all distinct: 1..150 times the smallest subnormal, +-(1 + j/8)
    sub = np.arange(1, 151, dtype=np.uint32).view(F32)
    big = (1 + np.arange(200) / 8.0).astype(F32)
    mixed = rng.permutation(np.r_[-big, -sub, sub, big, F32(1e-40), F32(-1e-40)].astype(F32))
    for what, k in (("neg_normal", 100), ("neg_subnormal", 275), ("last_negative", 351), ("first_positive", 352), ("pos_subnormal", 420),
                    ("pos_normal", 600)):
        add("mixed_" + what, mixed, k)
    inf = rng.permutation(np.r_[_distinct(300, 4), F32(-np.inf), F32(np.inf), F32(np.inf)].astype(F32))
    add("inf_first", inf, 1)
    add("inf_after_neginf", inf, 2)
    add("inf_before_posinf", inf, 301)
    add("inf_first_posinf", inf, 302)
    add("inf_last", inf, 303)
    nan = _distinct(n, 5).copy()
    nan[rng.choice(n, 77, replace=False)] = np.nan  # 700 numbers, then 77 NaN
    for what, k in (("below", 490), ("last_number", 700), ("first_nan", 701), ("inside", 740), ("last", n)):
        add("nan_" + what, nan, k)
    add("nan_and_inf", np.r_[inf, np.full(5, np.nan, F32)], 304)  # the first NaN follows +Inf
    add("all_nan", np.full(300, np.nan, F32), 200)
    add("one_nan", np.full(1, np.nan, F32), 1)
    # zeros of both signs between negative and positive numbers: 100 negatives, 150 x -0.0 and 150 x +0.0 mixed, 100 positives
    zeros = rng.permutation(np.r_[-big[:100], np.full(150, -0.0, F32), np.zeros(150, F32), big[:100]].astype(F32))
    add("zeros_last_negative", zeros, 100)
    add("zeros_first", zeros, 101, zero=True)
    add("zeros_lower_half", zeros, 180, zero=True)
    add("zeros_upper_half", zeros, 330, zero=True)
    add("zeros_last", zeros, 400, zero=True)
    add("zeros_first_positive", zeros, 401)
    # the second trip of k_sel_hist alone decides: the first 262 144 elements are all 2.0, the answer lies in the partial block after them
    tail = np.r_[np.full(HIST_SPAN, 2.0, F32), -(1 + np.arange(257, dtype=np.float64)).astype(F32)]
    add("second_trip_only", tail, 257)
    add("second_trip_count", tail, 258)
    return T


@functools.lru_cache(maxsize=None)
def selection_cases():
    """name -> (x, k, zero)."""
    return _sel_table()


SELECTION_NAMES = tuple(_sel_table())


# ---- the stopping function and the drivers ---------------------------------------------------------------------------------------

PATCH_SHAPE = (40, 50)
# (rows, cols) of the noise patch in the corner of the flat image whose Igrad zero count is the largest below, equal to and the smallest
# above the rank round(0.7*2000) = 1400; found by patch_search() and asserted by the CPU test
PATCH_BELOW, PATCH_EQUAL, PATCH_ABOVE = (10, 39), (8, 47), (8, 46)


def _noise(shape, C, seed):
    rng = np.random.default_rng([seed, shape[0], shape[1], C])
    return rng.uniform(0, 1, shape + ((C,) if C > 1 else ())).astype(F32)


def _flat(shape, C, v=0.25):
    return np.full(shape + ((C,) if C > 1 else ()), v, F32)


def patch_image(pr, pc, C=1, shape=PATCH_SHAPE):
    """Flat 0.25 with a pr x pc patch of noise in the top-left corner."""
    I = _flat(shape, C)
    I[:pr, :pc] = _noise((pr, pc), C, 7)
    return I


def box_phi(shape):
    """-1 with a box of +1 over the middle half, as runme.m draws its initial curve."""
    r, c = shape
    P = -np.ones(shape, F32)
    P[r // 4:max(r // 4 + 1, (3 * r) // 4), c // 4:max(c // 4 + 1, (3 * c) // 4)] = 1
    return P


def _images():
    T = {}

    def add(name, I):
        T[name] = _ro(I)

    for shape, C in (((3, 3), 1), ((3, 7), 2), ((7, 3), 3), ((5, 9), 1), ((5, 9), 3), ((65, 7), 3), ((7, 257), 2), ((255, 4), 1), ((257, 4), 3),
                     ((513, 512), 1)):
        add("noise_%dx%dx%d" % (shape + (C,)), _noise(shape, C, 11))
    i, j = np.mgrid[0:65, 0:7]
    add("binary_65x7x1", ((i // 4 + j // 4) % 2).astype(F32))  # 0/1 blocks of 4x4: Igrad repeats, so the sort is full of ties
    i, j, c = np.mgrid[0:33, 0:31, 0:3]
    add("binary_33x31x3", (((i + c) // 4 + j // 4) % 2).astype(F32))
    step = np.zeros((33, 31), F32)
    step[:, 15:] = 1
    add("step_33x31x1", step)  # most of Igrad is zero: lambda = 0
    add("flat_40x50x1", _flat(PATCH_SHAPE, 1))
    add("flat_5x9x2", _flat((5, 9), 2))
    add("patch8x8_40x50x1", patch_image(8, 8))
    add("patch21x21_40x50x1", patch_image(21, 21))
    for tag, p in (("below", PATCH_BELOW), ("equal", PATCH_EQUAL), ("above", PATCH_ABOVE)):
        if p is not None:
            add("patch%dx%d_zeros_%s_rank_40x50x1" % (p + (tag,)), patch_image(*p))
    I = _noise((65, 31), 1, 13)
    I[40, 20] = np.nan
    add("one_nan_65x31x1", I)
    I = _noise((33, 31), 3, 14)
    I[5, 6, 1] = np.nan
    add("one_nan_33x31x3", I)
    for c in (0, 1, 2):
        I = _noise((33, 31), 3, 15)
        I[:, :, c] = np.nan
        add("nan_channel%d_33x31x3" % c, I)
    I = _noise((9, 11), 2, 16)
    I[:] = np.nan
    add("all_nan_9x11x2", I)
    return T


@functools.lru_cache(maxsize=None)
def images():
    return _images()


IMAGE_NAMES = tuple(_images())
# name -> (image, lambda given to pdeip_gac_stopping_dev); -1: selected
STOPPING = tuple((n, -1.0) for n in IMAGE_NAMES) + (
    ("noise_65x7x3", 0.002), ("noise_65x7x3", 0.0), ("noise_65x7x3", 1e-40), ("noise_5x9x1", -0.0), ("flat_40x50x1", 0.002),
    ("one_nan_33x31x3", 0.002))


def stopping_id(c):
    return "%s-lambda_%g" % c if c[1] >= 0 and not np.signbit(c[1]) else ("%s-lambda_negzero" % c[0] if c[1] == 0 else c[0])


@functools.lru_cache(maxsize=None)
def want_stopping(image, lam):
    """(g, Igrad, lambda) of ref.gac_stopping."""
    g, Igrad, l = ref.gac_stopping(images()[image], lam)
    return _ro(g), _ro(Igrad), F32(l)


@functools.lru_cache(maxsize=None)
def patch_zero_count(pr, pc):
    _, Igrad, _ = ref.gac_stopping(patch_image(pr, pc), -1.0)
    return int((Igrad == 0).sum())


def patch_search():
    """-> (below, equal, above): the (rows, cols) patches whose zero count of Igrad is the largest below the rank, equal to it and the
    smallest above; among patches of one count the first in (rows, cols) order.  2000 stopping functions of 40x50: about two seconds."""
    k = driver_rank(PATCH_SHAPE[0] * PATCH_SHAPE[1])
    best = {"below": None, "equal": None, "above": None}
    for pr in range(1, PATCH_SHAPE[0] + 1):
        for pc in range(1, PATCH_SHAPE[1] + 1):
            z = patch_zero_count(pr, pc)
            if z < k and (best["below"] is None or z > best["below"][0]):
                best["below"] = (z, (pr, pc))
            if z == k and best["equal"] is None:
                best["equal"] = (z, (pr, pc))
            if z > k and (best["above"] is None or z < best["above"][0]):
                best["above"] = (z, (pr, pc))
    return tuple(None if best[t] is None else best[t][1] for t in ("below", "equal", "above"))


# A driver case: (image, models, parameters of ref.GAC).  `models` holds "a" only where its reference output is at least 75 % finite:
# with lambda = 0 or a NaN in g, model a's data term c*g*|grad PHI| is NaN everywhere and the whole of PHI floods, while model b's
# pos0 / neg0 and the harmonic mean drop the NaN.  For model a those inputs are pinned through pdeip_gac_stopping_dev (STOPPING).
DRIVER = (
    ("noise_3x3x1", "ab", dict(ITER=2)),
    ("noise_3x7x2", "ab", dict(ITER=2)),
    ("noise_7x3x3", "ab", dict(ITER=2)),
    ("noise_5x9x1", "ab", dict(ITER=2)),
    ("noise_5x9x3", "ab", dict(ITER=3, tau=0.1)),
    ("noise_65x7x3", "ab", dict(ITER=2)),
    ("noise_65x7x3", "a", dict(ITER=2, c=0.1)),
    ("noise_65x7x3", "a", dict(ITER=2, c=0.0)),
    ("noise_65x7x3", "ab", dict(ITER=2, lam=0.002, SMOOTH=1)),
    ("noise_65x7x3", "ab", dict(ITER=2, lam=0.0)),
    ("noise_65x7x3", "ab", dict(ITER=2, lam=1e-40)),
    ("noise_65x7x3", "ab", dict(ITER=0)),
    ("noise_65x7x3", "ab", dict(ITER=0.5)),
    ("noise_65x7x3", "ab", dict(ITER=2.5, tau=0.1, SMOOTH=1)),
    ("noise_7x257x2", "ab", dict(ITER=2)),
    ("noise_255x4x1", "ab", dict(ITER=2)),
    ("noise_257x4x3", "ab", dict(ITER=2)),
    ("noise_513x512x1", "ab", dict(ITER=1)),
    ("binary_65x7x1", "ab", dict(ITER=2)),
    ("binary_33x31x3", "ab", dict(ITER=2)),
    ("step_33x31x1", "b", dict(ITER=2)),
    ("flat_40x50x1", "b", dict(ITER=2)),
    ("flat_40x50x1", "ab", dict(ITER=2, lam=0.002)),
    ("patch8x8_40x50x1", "b", dict(ITER=2)),
    ("patch21x21_40x50x1", "ab", dict(ITER=2)),
    ("one_nan_65x31x1", "b", dict(ITER=2)),
    ("one_nan_33x31x3", "ab", dict(ITER=2)),
    ("nan_channel1_33x31x3", "ab", dict(ITER=2)),
) + tuple(("patch%dx%d_zeros_%s_rank_40x50x1" % (p + (tag,)), m, dict(ITER=2))
          for tag, p, m in (("below", PATCH_BELOW, "ab"), ("equal", PATCH_EQUAL, "b"), ("above", PATCH_ABOVE, "b")) if p is not None)
FLOOD = ("flat_40x50x1", "a", dict(ITER=2))  # the one driver case whose output is NaN everywhere, on both sides
DRIVER_RUNS = tuple((img, m, tuple(sorted(prm.items()))) for img, models, prm in DRIVER for m in models)


def driver_id(run):
    return "%s-%s-%s" % (run[0], run[1], "_".join("%s%g" % kv for kv in run[2]))


def phi_for(image):
    return _ro(box_phi(images()[image].shape[:2]))


@functools.lru_cache(maxsize=None)
def want_gac(image, model, prm):
    """ref.GAC of a driver run (prm: the sorted items of its parameters)."""
    return _ro(ref.GAC(images()[image], phi_for(image), model, **dict(prm)))


# ---- the line solves -------------------------------------------------------------------------------------------------------------

CHUNK = 8  # LS_CH / D4_CH: elements whose coefficients a line kernel fetches ahead of its chain
CHUNK_LENGTHS = (9, 10, 11, 18)  # n-2 = 7, 8, 9, 16 and n-1 = 8, 9, 10, 17
CHUNK_SHAPES = tuple((r, c) for r in CHUNK_LENGTHS for c in CHUNK_LENGTHS) + ((2, 18), (18, 2), (66, 10), (10, 66))
RANGE_SHAPE = (23, 19, 3)


def ac_problem(seed, shape, zero_diff=True):
    """PHI, D, GradNorm, Diff as the AC_solver_2d tests draw them (test_gpu_levelset.py), without NaN."""
    rng = np.random.default_rng(seed)
    phi = rng.uniform(-3, 3, shape).astype(F32)
    d = rng.uniform(-1, 1, shape).astype(F32)
    g = rng.uniform(0.0, 1.5, shape).astype(F32)
    diff = rng.uniform(0.0, 2.0, shape).astype(F32)
    diff[rng.random(shape) < 0.05] = 0  # interior zeros
    if zero_diff:
        diff[0, ...] = np.where(rng.random(diff[0].shape) < 0.5, 0, diff[0])
        diff[-1, ...] = np.where(rng.random(diff[-1].shape) < 0.5, 0, diff[-1])
        diff[:, 0] = np.where(rng.random(diff[:, 0].shape) < 0.5, 0, diff[:, 0])
        diff[:, -1] = np.where(rng.random(diff[:, -1].shape) < 0.5, 0, diff[:, -1])
    return [np.asfortranarray(x) for x in (phi, d, g, diff)]


def cv_problem(seed, shape):
    """PHI, D, DH, GradNorm as the CV_solver_2d tests draw them (test_gpu_cv.py), without NaN."""
    rng = np.random.default_rng(seed)
    phi = rng.uniform(-6, 6, shape).astype(F32)
    d = rng.uniform(-3, 3, shape).astype(F32)
    dh = rng.uniform(0.04, 0.32, shape).astype(F32)
    g = rng.uniform(0.0, 2.0, shape).astype(F32)
    g[rng.random(shape) < 0.04] = 0
    g[rng.random(shape) < 0.01] = F32(-0.0)
    g[0] = np.where(rng.random(g[0].shape) < 0.3, 0, g[0])
    g[-1] = np.where(rng.random(g[-1].shape) < 0.3, 0, g[-1])
    g[:, 0] = np.where(rng.random(g[:, 0].shape) < 0.3, 0, g[:, 0])
    g[:, -1] = np.where(rng.random(g[:, -1].shape) < 0.3, 0, g[:, -1])
    return [np.asfortranarray(x) for x in (phi, d, dh, g)]


def diff_image(seed, shape):
    """Piecewise-smooth 0..255 content as the Diffusion4_v10 tests draw it (test_gpu_diffusion.py)."""
    rng = np.random.default_rng(seed)
    blocks = rng.uniform(0, 255, (max(1, shape[0] // 16) + 1, max(1, shape[1] // 16) + 1) + tuple(shape[2:]))
    I = blocks[np.arange(shape[0]) // 16][:, np.arange(shape[1]) // 16] + rng.normal(0, 6, shape)
    return np.asfortranarray(np.clip(I, 0, 255).astype(F32))


@functools.lru_cache(maxsize=None)
def chunk_problem(family, shape):
    """The three-frame (three-channel) problem of a chunk-edge shape."""
    full = tuple(shape) + (3,)
    seed = 100 + 31 * shape[0] + shape[1]
    if family == "ac":
        return tuple(_ro(x) for x in ac_problem(seed, full))
    if family == "cv":
        return tuple(_ro(x) for x in cv_problem(seed, full))
    return (_ro(diff_image(seed, full)),)


AC_TAU_NU = (F32(0.25), F32(1.3))
CV_TAU_NU = (F32(0.5), F32(0.3))
PLANES = {"ac": ("PHI", "D", "GN", "Diff"), "cv": ("PHI", "D", "DH", "G")}
# (plane, value, how): "laced" = 3 % of the plane's pixels in every frame; "pixel" = one interior pixel of the middle frame, for the
# values that flood the lines they touch (frames are independent in both solvers, and the other lines stay informative)
_ORD = ((0, -0.0), (0, 1e-20), (0, -1.0), (1, 1e-40), (1, -1e-40), (1, -0.0), (1, 1e-20), (1, -1.0),
        (2, 1e-40), (2, -1e-40), (2, -0.0), (2, 1e-20), (2, 1e20), (2, -1.0),
        (3, -1e-40), (3, -0.0), (3, 3e38), (3, -3e38), (3, np.inf), (3, 1e20), (3, -1.0))
_FLOOD = ((0, 3e38), (0, -3e38), (0, np.inf), (0, 1e20), (1, 3e38), (1, -3e38), (1, np.inf), (1, 1e20),
          (2, 3e38), (2, -3e38), (2, np.inf), (3, 1e-40), (3, 1e-20))
RANGE_CASES = tuple((p, v, "laced") for p, v in _ORD) + tuple((p, v, "pixel") for p, v in _FLOOD)
TAU_NU_CASES = ((0.0, 1.3), (0.25, 0.0), (-0.25, 1.3), (0.25, -1.3), (1e-40, 1.0), (1e-30, 1e-30))
RANGE_PIXEL = (11, 8, 1)


def range_id(c):
    return "%d_%g_%s" % (c[0], c[1], c[2]) if not (c[1] == 0 and np.signbit(c[1])) else "%d_negzero_%s" % (c[0], c[2])


@functools.lru_cache(maxsize=None)
def range_problem(family, plane, value, how):
    """The ordinary 23x19x3 problem of the family with `value` written into plane number `plane`.  One uniform plane decides the
    laced pixels, as range_problems.py does."""
    base = ac_problem(201, RANGE_SHAPE, zero_diff=False) if family == "ac" else cv_problem(202, RANGE_SHAPE)
    a = base[plane]
    if how == "laced":
        u = np.random.default_rng([203, 0x72616e67]).uniform(size=RANGE_SHAPE[:2])
        a[u < 0.03] = F32(value)
    else:
        a[RANGE_PIXEL] = F32(value)
    return tuple(_ro(x) for x in base)


@functools.lru_cache(maxsize=None)
def range_base(family):
    base = ac_problem(201, RANGE_SHAPE, zero_diff=False) if family == "ac" else cv_problem(202, RANGE_SHAPE)
    return tuple(_ro(x) for x in base)


def solve_ref(family, prob, tau, nu):
    fn = ref.AC_solver_2d if family == "ac" else cv_ref.CV_solver_2d
    return fn(*prob, F32(tau), F32(nu))


# Diffusion4_v10: the channels share their weights, so there is no frame trick; these values keep the output finite at 1 % lacing
DIFF_SHAPE = (19, 23, 3)
DIFF_VALUES = (1e20, 3e38, 1e-40, -0.0, -50.0, 1e5)
DIFF_ALPHAS = (0.0, 1e-30, -1.0, -20.0)  # alpha >= 1e10 makes every system numerically singular: left out
DIFF_PIXEL = (7, 9, 1)


@functools.lru_cache(maxsize=None)
def diff_laced(value):
    I = diff_image(301, DIFF_SHAPE)
    u = np.random.default_rng([302, 0x72616e67]).uniform(size=DIFF_SHAPE[:2])
    I[u < 0.01] = F32(value)  # every channel of the pixel
    return _ro(I)


@functools.lru_cache(maxsize=None)
def diff_one_pixel(value):
    """NaN or +Inf on ONE pixel of ONE channel: with outer_iter = 0 (one iteration) the weights stay finite -- max(., [], 3) drops
    the NaN, and 1/sqrt(Inf) is 0 -- so that only the two lines through the pixel carry it.  The pixel is in channel 1, the one
    place where the .m's maximum and the DdiffWeights gateway's (which keeps a NaN of frame 0) agree; diffusion_nan_cases.py has the
    pixel in every channel."""
    I = diff_image(303, DIFF_SHAPE)
    I[DIFF_PIXEL] = F32(value)
    return _ro(I)


@functools.lru_cache(maxsize=None)
def diff_flat():
    """A flat image does not come back flat: with every gradient 0 the weights are 1/sqrt(1e-5) = 316.2, alpha*w is about 7906 beside
    the 2 of the diagonal, and each Thomas solve of the constant right-hand side loses a few units of the last place per element to
    that ratio.  The statement in single moves 77.25 by up to 0.012 over the six iterations; the GPU must reproduce those bits."""
    return _ro(np.full(DIFF_SHAPE, 77.25, F32))


# Reinit: a single step (T = 0.25) does not carry a NaN beyond radius 1
REINIT_SHAPE = (37, 29)
REINIT_STEP_VALUES = (1e20, -1e20, 1e-40, -1e-40, 0.0, -0.0, np.inf, -np.inf, 3e38)  # 1e20: the square overflows
REINIT_LONG_VALUES = (1e-40, -1e-40, 1e-45, 0.0, -0.0, 1e18, -1e18)                  # no NaN: these run at T = 10


def _reinit_laced(values, seed):
    rng = np.random.default_rng(seed)
    phi = rng.uniform(-4, 4, REINIT_SHAPE).astype(F32)
    u = np.random.default_rng([seed, 0x72616e67]).uniform(size=REINIT_SHAPE)
    for k, v in enumerate(values):
        phi[(u >= 0.01 * k) & (u < 0.01 * (k + 1))] = F32(v)
    return _ro(phi)


@functools.lru_cache(maxsize=None)
def reinit_step_case():
    return _reinit_laced(REINIT_STEP_VALUES, 401)


@functools.lru_cache(maxsize=None)
def reinit_long_case():
    return _reinit_laced(REINIT_LONG_VALUES, 402)


def finite_share(a):
    return float(np.isfinite(a).mean())
