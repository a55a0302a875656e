"""The inputs of the MATLAB-side stage tests (tests/test_gpu_stage_edges.py), each chosen for one way a stage kernel can go wrong,
and the functions that say what a case contains.  tests/test_stage_edge_cases.py proves on the CPU that every case is what its name
says; without that a case could pass while testing nothing.  Arrays are MATLAB-shaped float32 [rows, cols(, F)], built once per
process and read-only."""
import functools
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32

# pdeip_tv.hpp / tv_select_lambda: a thin histogram pass takes 4 096 norms per workgroup, a fat one 16 384
SEAM_SHAPES = ((64, 64), (17, 241), (128, 128), (113, 145), (200, 200))
TIE_RUN = 64  # a tie case: the wanted rank lies in a run of at least this many equal norms


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


# ---- median --------------------------------------------------------------------------------------------------------------------

NAN_COUNTS = (0, 1, 4, 5, 9)
MEDIAN_KINDS = tuple("nan%d" % k for k in NAN_COUNTS) + ("posinf", "neginf", "inf_below_nan", "all_equal", "distinct456", "mixed_zero",
                                                         "mixed_zero_median", "nan_on_borders", "nan_in_corners")


def windows(S):
    """The nine values of every 3x3 window with symmetric padding: [9, rows, cols], in the kernel's order (columns outer)."""
    P = np.pad(np.asarray(S, dtype=F32), 1, mode="symmetric")
    rows, cols = S.shape
    return np.stack([P[di:di + rows, dj:dj + cols] for dj in range(3) for di in range(3)], axis=0)


def mixed_zero_median(S):
    """Where the window holds zeros of both signs and its median is a zero: the one place where only the value is defined."""
    W = windows(S)
    zero = W == 0
    both = (zero & np.signbit(W)).any(axis=0) & (zero & ~np.signbit(W)).any(axis=0)
    return both & (np.sort(W, axis=0)[4] == 0)


def median_kinds(S):
    """Which of MEDIAN_KINDS the windows of S contain."""
    W = windows(S)
    rows, cols = S.shape
    nan = np.isnan(W)
    cnt = nan.sum(axis=0)
    srt = np.sort(W, axis=0)
    zero = W == 0
    both = (zero & np.signbit(W)).any(axis=0) & (zero & ~np.signbit(W)).any(axis=0)
    out = {"nan%d" % k for k in range(10) if (cnt == k).any()}
    with np.errstate(invalid="ignore"):
        if (W == np.inf).any():
            out.add("posinf")
        if (W == -np.inf).any():
            out.add("neginf")
        if ((srt[4] == np.inf) & (cnt > 0)).any():
            out.add("inf_below_nan")
        if ((W == W[0]).all(axis=0)).any():
            out.add("all_equal")
        if ((srt[3] < srt[4]) & (srt[4] < srt[5])).any():
            out.add("distinct456")
    if both.any():
        out.add("mixed_zero")
    if (both & (srt[4] == 0)).any():
        out.add("mixed_zero_median")
    part = (cnt >= 1) & (cnt <= 8)  # the window mixes NaN and numbers
    if rows >= 3 and cols >= 3:
        if part[0, 1:-1].any() and part[-1, 1:-1].any() and part[1:-1, 0].any() and part[1:-1, -1].any():
            out.add("nan_on_borders")
        if part[0, 0] and part[0, -1] and part[-1, 0] and part[-1, -1]:
            out.add("nan_in_corners")
    return out


def _plant_nan_counts(S, r, c, step_r, step_c):
    """Windows with exactly 1, 4, 5 and 9 NaN: a single NaN, a 2x2 block, a plus and a 3x3 block, three columns wide each, placed
    from (r, c) on in steps of (step_r, step_c); rows r-1 .. and columns c-1 .. must exist around each."""
    S[r, c] = np.nan                                                   # 1
    r, c = r + step_r, c + step_c
    S[r:r + 2, c - 1:c + 1] = np.nan                                   # 4 (the window centred on (r, c) holds the block)
    r, c = r + step_r, c + step_c
    S[r, c - 1:c + 2] = np.nan                                         # 5: the plus
    S[r - 1:r + 2, c] = np.nan
    r, c = r + step_r, c + step_c
    S[r - 1:r + 2, c - 1:c + 2] = np.nan                               # 9


def _split_sum(S, rng):
    """A, B with single(A + B) == S bit for bit: about half of the numbers are S - R and R for a random quarter R wherever that sum is
    exact, the others meet -0 (x + -0 = x for every x, -0 included); NaN come from Inf - Inf or from a NaN term; Inf from Inf + 3."""
    S = np.asarray(S, dtype=F32)
    A, B = S.copy(), np.full(S.shape, -0.0, F32)
    R = (rng.integers(1, 9, S.shape) * rng.choice([-0.25, 0.25], S.shape)).astype(F32)
    with np.errstate(invalid="ignore"):
        D = (S - R).astype(F32)
        back = (D + R).astype(F32)
    cut = np.isfinite(S) & (S != 0) & (back.view(np.uint32) == S.view(np.uint32)) & (rng.random(S.shape) < 0.5)
    A[cut], B[cut] = D[cut], R[cut]
    nan = np.isnan(S)
    inf_minus_inf = nan & (rng.random(S.shape) < 0.5)
    A[inf_minus_inf], B[inf_minus_inf] = np.inf, -np.inf
    B[nan & ~inf_minus_inf] = 1.0
    B[np.isinf(S)] = 3.0
    return A, B


@functools.lru_cache(maxsize=None)
def median_cases():
    """(name, S, A, B, kinds): S the frame that is filtered, A + B == S its two-term form, kinds what the case claims to contain."""
    out = []

    def add(name, S, kinds, seed):
        A, B = _split_sum(S, np.random.default_rng(seed))
        out.append((name, _ro(S), _ro(A), _ro(B), frozenset(kinds)))

    all_counts = {"nan%d" % k for k in NAN_COUNTS}
    # every NaN count among distinct numbers; partial windows on every border and in every corner
    rng = np.random.default_rng(101)
    S = rng.uniform(-2, 2, (23, 21)).astype(F32)
    _plant_nan_counts(S, 3, 10, 5, 0)
    S[0, 5] = S[-1, 7] = S[6, 0] = S[9, -1] = np.nan
    S[1, 1] = S[1, -2] = S[-2, 1] = S[-2, -2] = np.nan
    add("nan_counts_23x21", S, all_counts | {"distinct456", "nan_on_borders", "nan_in_corners"}, 1)
    # the same in a frame that crosses the 256-row block of the pixel index, three columns wide
    S = rng.uniform(-2, 2, (300, 3)).astype(F32)
    _plant_nan_counts(S, 250, 1, 5, 0)
    S[0, 1] = S[-1, 1] = S[100, 0] = S[120, 2] = np.nan
    add("nan_counts_300x3", S, all_counts | {"distinct456", "nan_on_borders"}, 2)
    S = rng.uniform(-2, 2, (3, 40)).astype(F32)
    _plant_nan_counts(S, 1, 5, 0, 6)
    add("nan_counts_3x40", S, all_counts | {"distinct456"}, 3)
    # a third of the pixels NaN, and a block for the all-NaN window
    S = rng.uniform(-2, 2, (37, 53)).astype(F32)
    S[rng.random(S.shape) < 0.33] = np.nan
    S[20:23, 30:33] = np.nan
    S[5:8, 5:8] = rng.uniform(-2, 2, (3, 3))
    add("nan_lace_37x53", S, all_counts | {"distinct456", "nan_on_borders"}, 4)
    # +Inf and -Inf: alone, together, and +Inf as the 5th value below four NaN (NaN orders above +Inf)
    S = rng.uniform(-2, 2, (19, 22)).astype(F32)
    S[3, 3], S[3, 10], S[8, 5], S[8, 6] = np.inf, -np.inf, np.inf, -np.inf
    S[12:14, 9:11] = np.nan
    S[12:15, 11] = np.inf
    S[0, 15] = S[-1, 15] = -np.inf
    add("inf_19x22", S, {"posinf", "neginf", "inf_below_nan", "nan0", "nan4"}, 5)
    # ties: flat plateaus (all nine equal) in an integer-valued frame
    S = rng.integers(0, 4, (20, 25)).astype(F32)
    S[4:10, 6:13] = 2.0
    S[0:4, 0:4] = 3.0
    add("plateaus_20x25", S, {"all_equal", "nan0"}, 6)
    # zeros of both signs among small numbers: many windows whose median is a zero of either sign
    S = rng.choice(np.array([0.0, -0.0, 0.0, -0.0, -1.0, 1.0, 1e-45, -1e-45], F32), size=(18, 17))
    add("signed_zeros_18x17", S, {"mixed_zero", "mixed_zero_median", "nan0"}, 7)
    # the smallest frame: one NaN in the middle is in every window exactly once
    S = rng.uniform(-2, 2, (3, 3)).astype(F32)
    S[1, 1] = np.nan
    add("min_3x3", S, {"nan1"}, 8)
    return tuple(out)


def median_names():
    return [c[0] for c in median_cases()]


def median_case(name):
    return {c[0]: c for c in median_cases()}[name]


def median_model(S):
    """The kernel's 19-exchange network with its exchange rule (a > b, or a is NaN), vectorised over the frame: shows on the CPU that
    the network with this rule selects the 5th value of the NaN-last order."""
    v = list(windows(S))

    def cswap(a, b):
        with np.errstate(invalid="ignore"):
            ex = (v[a] > v[b]) | np.isnan(v[a])
        v[a], v[b] = np.where(ex, v[b], v[a]), np.where(ex, v[a], v[b])

    for a, b in ((1, 2), (4, 5), (7, 8), (0, 1), (3, 4), (6, 7), (1, 2), (4, 5), (7, 8), (0, 3), (5, 8), (4, 7), (3, 6), (1, 4), (2, 5), (4, 7),
                 (4, 2), (6, 4), (4, 2)):
        cswap(a, b)
    return v[4]


# ---- selection of lambda ---------------------------------------------------------------------------------------------------------

def _random_image(seed, shape):
    return np.random.default_rng(seed).uniform(0, 1, shape).astype(F32)


def _edge_image(shape):
    """Two values, one straight edge along the longer side: every non-zero norm is the same number."""
    rows, cols = shape
    I = np.zeros(shape, F32)
    if rows >= cols:
        I[:, cols // 2:] = 255.0
    else:
        I[rows // 2:, :] = 255.0
    return I


def _blocks_image(seed, shape):
    """Two values in random 8x8 blocks: a handful of distinct norms (straight edges, corners), each in a long run."""
    rows, cols = shape
    b = np.random.default_rng(seed).integers(0, 2, ((rows + 7) // 8, (cols + 7) // 8))
    return (255.0 * np.kron(b, np.ones((8, 8)))[:rows, :cols]).astype(F32)


def _impulse_frames(seed, shape):
    """Three frames whose strongest frame changes from pixel to pixel (independent textures under independent smooth envelopes),
    with a flat field in which single-pixel impulses make EXACT ties between the frames: at the pixel diagonally between them an
    impulse of height h gives (dx, dy) = (k1 h, k1 h), (-k1 h, k1 h), (k1 h, -k1 h) in frames 0, 1, 2 -- one norm, but the sign of
    dx*dy (and with it the diagonal weights) tells which frame was taken.  The first frame must win."""
    rows, cols = shape
    rng = np.random.default_rng(seed)
    jj, ii = np.meshgrid(np.arange(cols), np.arange(rows))
    D = np.stack([rng.uniform(0, 1, shape) * (0.6 + 0.5 * np.sin(0.37 * ii + 2.1 * f) * np.cos(0.29 * jj - 1.3 * f)) for f in range(3)], axis=2)
    D = D.astype(F32)
    D[8:40, 8:40, :] = 0.0
    for k, (p, q) in enumerate([(12, 12), (12, 20), (12, 28), (20, 12), (20, 20), (20, 28), (28, 12), (28, 20), (28, 28)]):
        h = F32(0.5 + 0.25 * k)
        order = (k, k + 1, k + 2)  # which frame gets which of the three impulses around the pixel (p, q)
        D[p + 1, q + 1, order[0] % 3] = h
        D[p + 1, q - 1, order[1] % 3] = h
        D[p - 1, q + 1, order[2] % 3] = h
    return D


def selection_info(D, quantile):
    """What the numpy statement selects on D: the sorted non-zero norms, the 1-based rank, lambda, and the pieces to restate the
    weights with another lambda."""
    ms = matlab_side()
    mx, my, norm = ms.ad_strongest(*ms.ad_frame_gradients(D))
    srt = ms.ad_sorted_nonzero(norm)
    rank = ms.ad_rank(srt.size, quantile) if srt.size else 0
    return dict(mx=mx, my=my, norm=norm, sorted=srt, rank=rank, lam=srt[rank - 1] if srt.size else 1.0)


def weights_with(info, lam, quantile, alpha=None):
    """The eight single weight planes the stage returns, from lambda `lam`: the flow driver's form for a quantile, the denoiser's
    (alpha-scaled, borders zeroed) for quantile None."""
    ms = matlab_side()
    w = ms.ad_tensor_weights(info["mx"], info["my"], info["norm"], lam, wrap=quantile is not None)
    return [(a if quantile is not None else alpha * a).astype(F32) for a in w]


def classify(D, quantile, alpha=500.0):
    """'rank': the norms next to the wanted rank (both, or the one there is at either end of the list) differ from the one at the rank,
    and each of them as lambda changes bits of a weight plane; 'tie': the wanted rank lies in a run of at least TIE_RUN equal
    norms; otherwise None."""
    info = selection_info(D, quantile)
    srt, r = info["sorted"], info["rank"]
    if srt.size == 0:
        return None
    lam = srt[r - 1]
    if int((srt == lam).sum()) >= TIE_RUN:
        return "tie"
    others = ([srt[r - 2]] if r >= 2 else []) + ([srt[r]] if r <= srt.size - 1 else [])
    if not others or any(o == lam for o in others):
        return None
    base = weights_with(info, lam, quantile, alpha)
    for other in others:
        w = weights_with(info, other, quantile, alpha)
        if all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(base, w)):
            return None
    return "rank"


def crossing_quantiles(count, k):
    """Two adjacent doubles q_below < q_above around (k - 0.5) / count with floor(count*q + 0.5) == k - 1 and == k."""
    rank = lambda q: int(np.floor(count * q + 0.5))
    q = (k - 0.5) / count
    while rank(q) >= k:
        q = np.nextafter(q, 0.0)
    while rank(np.nextafter(q, 1.0)) < k:
        q = np.nextafter(q, 1.0)
    return float(q), float(np.nextafter(q, 1.0))


@functools.lru_cache(maxsize=None)
def selection_cases():
    """(name, D, quantile, cls): quantile None is the denoiser's median form (tv_assemble), a number the flow driver's (ad_weights).
    Every seam size carries a rank-sensitive and a tie image in both forms."""
    out = []
    for k, shape in enumerate(SEAM_SHAPES):
        tag = "%dx%d" % shape
        rnd, edge = _ro(_random_image(300 + k, shape)), _ro(_edge_image(shape))
        for q in (None, 0.9):
            out.append(("random_%s_%s" % (tag, "median" if q is None else "q90"), rnd, q, "rank"))
            out.append(("edge_%s_%s" % (tag, "median" if q is None else "q90"), edge, q, "tie"))
    for k, shape in enumerate(((113, 145), (200, 200))):
        blocks = _ro(_blocks_image(320 + k, shape))
        out.append(("blocks_%dx%d_median" % shape, blocks, None, "tie"))
        out.append(("blocks_%dx%d_q75" % shape, blocks, 0.75, "tie"))
    # the ends of the rank: the largest norm, the rank clamped to 1, and n*q + 0.5 crossing an integer between two adjacent doubles
    shape = (113, 145)
    rnd = _ro(_random_image(303, shape))
    count = int(selection_info(rnd, 0.5)["sorted"].size)
    below, above = crossing_quantiles(count, 7001)
    for name, q in (("q_one", 1.0), ("q_clamped", 1e-9), ("q_below_crossing", below), ("q_above_crossing", above)):
        out.append(("random_113x145_%s" % name, rnd, q, "rank"))
    # a flat image that is not zero: dx cancels exactly, dy leaves a rounding residue (k1 a + k2 a + k1 a - k1 a - k2 a - k1 a, left
    # to right), so lambda is that residue, the same at every pixel, and not 1
    out.append(("flat_residue_128x128_q90", _ro(np.full((128, 128), 0.375, F32)), 0.9, "tie"))
    out.append(("flat_residue_128x128_median", _ro(np.full((128, 128), 0.375, F32)), None, "tie"))
    frames = _ro(_impulse_frames(330, (113, 145)))
    out.append(("frames3_113x145_q90", frames, 0.9, "rank"))
    out.append(("frames3_113x145_median", frames, None, "rank"))
    return tuple(out)


def selection_names():
    return [c[0] for c in selection_cases()]


def selection_case(name):
    return {c[0]: c for c in selection_cases()}[name]


@functools.lru_cache(maxsize=None)
def degenerate_cases():
    """(name, D, nonzero): images with `nonzero` non-zero norms -- none (lambda = 1) or those of one pixel's neighbourhood."""
    out = []
    for shape in ((17, 241), (128, 128)):
        flat = np.zeros(shape, F32)
        out.append(("flat_%dx%d" % shape, _ro(flat), 0))
        bump = flat.copy()
        bump[shape[0] // 2, shape[1] // 3] = 1.0
        out.append(("bump_%dx%d" % shape, _ro(bump), 8))  # the eight neighbours; at the pixel itself the derivative cancels
    return tuple(out)


@functools.lru_cache(maxsize=None)
def nonfinite_cases():
    """(name, D, what): frames with NaN / Inf pixels for ad_weights, tv_assemble and tv4_assemble.  `what` names the frame maximum
    each one decides: 'all' -- a pixel NaN in every frame (or in the only one) must carry NaN into the selection; 'some' -- a NaN in
    some frames only is skipped like MATLAB's max skips it; 'inf' -- +Inf pixels (Inf - Inf in the derivative)."""
    rng = np.random.default_rng(340)
    out = []
    one = rng.uniform(0, 1, (64, 64)).astype(F32)
    one[10, 12] = one[40, 41] = one[0, 0] = np.nan
    out.append(("nan_single_frame_64x64", _ro(one), "all"))
    three = rng.uniform(0, 1, (64, 67, 3)).astype(F32)
    some = three.copy()
    some[10, 12, 1] = some[30, 31, 0] = some[50, 5, 2] = some[63, 66, 0] = np.nan
    some[20, 40, 0] = some[20, 40, 1] = np.nan
    out.append(("nan_some_frames_64x67x3", _ro(some), "some"))
    every = three.copy()
    every[10, 12, :] = every[33, 0, :] = np.nan
    every[50, 50, 2] = np.nan
    out.append(("nan_every_frame_64x67x3", _ro(every), "all"))
    inf = rng.uniform(0, 1, (64, 67, 2)).astype(F32)
    inf[12, 13, 0] = inf[40, 20, 1] = np.inf
    inf[40, 22, 1] = np.inf      # between the two, k2*Inf - k2*Inf: a NaN derivative from numbers that are not NaN
    inf[5, 50, 0] = -np.inf
    out.append(("inf_64x67x2", _ro(inf), "inf"))
    return tuple(out)


# ---- warps -------------------------------------------------------------------------------------------------------------------------

def ulp_up(x):
    return np.nextafter(F32(x), F32(np.inf))


def ulp_down(x):
    return np.nextafter(F32(x), F32(-np.inf))


@functools.lru_cache(maxsize=None)
def sym_warp_cases():
    """(name, U, Uq) for sym_warp_flow: the query is (j + 1) + Uq in double.  Row r of Uq puts one kind of query into every column:
    0 exactly column 1, 1 exactly the last column, 2 / 3 one single-precision ulp outside either end (NaN), 4 / 5 one ulp inside,
    6 exact integers in the interior, 7 NaN, 8 / 9 +-Inf, the rest random."""
    out = []
    for rows, cols in ((12, 37), (300, 3), (3, 9)):
        rng = np.random.default_rng(rows + cols)
        U = rng.uniform(-2, 2, (rows, cols)).astype(F32)
        Uq = rng.uniform(-3, 3, (rows, cols)).astype(F32)
        col = np.arange(1, cols + 1, dtype=np.float64)
        rowsets = [F32(1.0) - col, F32(cols) - col, ulp_down(1.0) - col, ulp_up(cols) - col, ulp_up(1.0) - col, ulp_down(cols) - col,
                   ((np.arange(cols) * 7) % cols + 1) - col]
        for r, q in enumerate(rowsets[:min(rows, 7)]):
            Uq[r % rows, :] = q.astype(F32)
        if rows > 9:
            Uq[7, :], Uq[8, :], Uq[9, :] = np.nan, np.inf, -np.inf
        else:
            Uq[0, 0], Uq[1, 1], Uq[2, 2] = np.nan, np.inf, -np.inf
        out.append(("%dx%d" % (rows, cols), _ro(U), _ro(Uq)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def flow_warp_cases():
    """(name, U, V) for flow_warp against flow_coords + warp_bilinear: single(j + 1 + U) is an exact integer in row 0, exactly the
    last column in row 1, one ulp past it in row 2, one ulp before column 1 in row 3; rows of V likewise in columns 0..3; random
    elsewhere, with NaN and Inf."""
    out = []
    for rows, cols in ((37, 53), (300, 5), (5, 7)):
        rng = np.random.default_rng(rows * cols)
        U = rng.uniform(-3, 3, (rows, cols)).astype(F32)
        V = rng.uniform(-3, 3, (rows, cols)).astype(F32)
        col, row = np.arange(1, cols + 1, dtype=F32), np.arange(1, rows + 1, dtype=F32)
        U[0, :] = ((np.arange(cols) * 3) % cols + 1).astype(F32) - col
        U[1, :] = F32(cols) - col
        U[2, :] = ulp_up(cols) - col
        U[3, :] = ulp_down(1.0) - col
        V[:, 0] = ((np.arange(rows) * 3) % rows + 1).astype(F32) - row
        V[:, 1] = F32(rows) - row
        V[:, 2] = ulp_up(rows) - row
        V[:, 3] = ulp_down(1.0) - row
        U[4, 4], V[6 % rows, 4] = np.nan, np.inf
        out.append(("%dx%d" % (rows, cols), _ro(U), _ro(V)))
    return tuple(out)
