"""Cases for the flow tools' reductions and flat kernels, chosen from the constants of their loops and not from field content: the
shapes at which a final thread folds a second partial, runs its batched loop, hands over to its tail loop; the sizes at which the
flow errors' final pass takes a second round of tiles, the maximum's kernel and the flat sweeps a second stride.  Two value families
per shape: `integers` (every sum exact in any order: a wrong result is an omitted or doubled partial, or the division) and `binades`
(magnitudes m 2^e, e uniform in -20..20: a fold in another order gives other bits).  tests/test_flow_round_cases.py proves on the
CPU that each case reaches what it claims; tests/test_gpu_flow_rounds.py runs them.  Planes are read-only; the caches are small,
since a test asks for its case once and the largest planes have a million pixels."""
import functools
import zlib

import numpy as np

import crosscheck_ref as cr
import flowviz_ref as fr
import reduce_tree_ref as rt

F32, F64 = np.float32, np.float64

# name: (value, the line it mirrors)
CONSTANTS = {
    "BLOCK": (256, "csrc/pdeip_crosscheck.hpp, pdeip_flowviz.hpp, pdeip_interp.hpp: constexpr int BLOCK = 256; FLAT_BLOCK of pdeip_inpaint.hpp"),
    "FINAL_BLOCK": (1024, "csrc/pdeip_crosscheck.hpp: constexpr int FINAL_BLOCK = 1024"),
    "FINAL_BATCH": (4, "csrc/pdeip_crosscheck.hpp: constexpr int FINAL_BATCH = 4"),
    "ERR_TILE": (2048, "csrc/pdeip_flowviz.hpp: constexpr int ERR_TILE = BLOCK * ERR_PER_THREAD (256 * 8)"),
    "MAXMAG_BLOCKS": (1024, "csrc/pdeip_flowviz.hpp: constexpr int MAXMAG_BLOCKS = 1024"),
    "FLAT_BLOCKS": (256 * 16, "csrc/pdeip_interp.hip, pdeip_inpaint.hip: if (blocks > 256 * 16) blocks = 256 * 16"),
}
BLOCK, FINAL_BLOCK, FINAL_BATCH, ERR_TILE, MAXMAG_BLOCKS, FLAT_BLOCKS = (CONSTANTS[k][0] for k in (
    "BLOCK", "FINAL_BLOCK", "FINAL_BATCH", "ERR_TILE", "MAXMAG_BLOCKS", "FLAT_BLOCKS"))
FAMILIES = ("integers", "binades")


def _frozen(a):
    a = np.asfortranarray(np.asarray(a, dtype=F32))
    a.setflags(write=False)
    return a


def _seed(*key):
    return zlib.crc32(repr(key).encode())


# ---- the cross-checks ------------------------------------------------------------------------------------------------------------
# nparts each side of one stride of the final workgroup (1024), of the batched loop's bound (3 * 1024) and of one batch (4096); 7168
# is the one size at which thread 0 runs a batch and then three tail steps (7169 gives it two batches), 7169 that size for thread
# 1023, 8193 two batches and a tail.
NPARTS = (1024, 1025, 3072, 3073, 4096, 4097, 7168, 7169, 8193)
TALL_SHAPES = ((257, 1537), (513, 1366))   # two row blocks, 3074 parts, every second part one live row; three row blocks, 4098 parts
CROSS_SHAPES = tuple((1, n) for n in NPARTS) + tuple((2, n) for n in NPARTS) + TALL_SHAPES
SWEEP_SHAPE = (2, 7169)
SWEEP_PARTS = (0, 1023, 1024, 3071, 3072, 4095, 4096, 5119, 7167, 7168)   # 5119, 7167: the first and the last tail step of thread 1023
SWEEP_VALUE = 1000.0
DISP_TOL = {"integers": 3.0, "binades": 1.0}
FLOW_AB = {"integers": (0.0, 30.0), "binades": (0.0, 1.0)}
PYTHAGOREAN = ((0, 0), (1, 0), (0, -2), (3, 4), (-4, 3), (5, 12), (-8, 6), (0, 7))   # (ub, vb): |.| = 0, 1, 2, 5, 5, 13, 10, 7
# A binades case whose restated mean has the bits of a wrong order pins nothing: it gets another seed here (test_reduce_tree_ref.py
# checks every one).  (what, shape) or ("err", n, masked, dead_from_tile): attempt
RESEED = {
    ('disp', (1, 1024)): 1,
    ('disp', (1, 1025)): 4,
    ('disp', (1, 3072)): 6,
    ('disp', (1, 3073)): 27,
    ('disp', (1, 4096)): 63,
    ('disp', (1, 4097)): 2,
    ('disp', (1, 7168)): 138,
    ('disp', (1, 7169)): 9,
    ('disp', (1, 8193)): 1,
    ('disp', (2, 1024)): 12,
    ('disp', (2, 1025)): 10,
    ('disp', (2, 3072)): 8,
    ('disp', (2, 3073)): 3,
    ('disp', (2, 4096)): 20,
    ('disp', (2, 4097)): 51,
    ('disp', (2, 7168)): 13,
    ('disp', (2, 7169)): 40,
    ('disp', (2, 8193)): 30,
    ('disp', (257, 1537)): 9,
    ('disp', (513, 1366)): 47,
    ('flow', (2, 1024)): 30,
    ('flow', (2, 1025)): 1,
    ('flow', (2, 3073)): 7,
    ('flow', (2, 4096)): 7,
    ('flow', (2, 4097)): 24,
    ('flow', (2, 7168)): 3,
    ('flow', (2, 7169)): 202,
    ('flow', (2, 8193)): 21,
    ('flow', (257, 1537)): 1,
    ('flow', (513, 1366)): 76,
    ('err', 524288, False, None): 32,
    ('err', 524289, False, None): 3,
    ('err', 524289, True, None): 6,
    ('err', 1048576, False, None): 25,
    ('err', 1048576, True, None): 13,
    ('err', 1048577, True, None): 9,
}


def shapes_of(what):
    """Disparity takes nrows >= 1, flow nrows >= 2."""
    return tuple(s for s in CROSS_SHAPES if what == "disp" or s[0] >= 2)


def nparts_of(shape):
    return shape[1] * ((shape[0] + BLOCK - 1) // BLOCK)


def final_iterations(nparts, t):
    """(batched, tail) iterations of thread t of k_crosscheck_final, from its loop bounds."""
    p, batched, tail = t, 0, 0
    while p < nparts - (FINAL_BATCH - 1) * FINAL_BLOCK:
        batched += 1
        p += FINAL_BATCH * FINAL_BLOCK
    while p < nparts:
        tail += 1
        p += FINAL_BLOCK
    return batched, tail


def _binade_values(rng, shape):
    m = 1.0 + rng.integers(0, 1 << 23, size=shape).astype(F64) * 2.0 ** -23   # [1, 2), exact in float32
    e = rng.integers(-20, 21, size=shape)
    sign = np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    return (sign * np.ldexp(m, e)).astype(F32)


def _holes(rng, shape, count=5):
    """A few pixels to make undefined, the first and the last among them."""
    n = shape[0] * shape[1]
    return sorted({0, n - 1} | set(int(p) for p in rng.integers(0, n, size=count)))


@functools.lru_cache(maxsize=4)
def disp_case(shape, family, largest_at=None):
    """-> D0, D1, tol.  D0 = 0, so the residual of a pixel is D1 there (and NaN where D1 or its right-hand neighbour is NaN)."""
    rng = np.random.default_rng(_seed("disp", shape, family, RESEED.get(("disp", shape), 0) if family == "binades" else 0))
    if family == "integers":
        D1 = rng.integers(-7, 8, size=shape).astype(F32)
    else:
        D1 = _binade_values(rng, shape)
    D1 = np.asfortranarray(D1)
    if largest_at is None:
        D1.reshape(-1, order="F")[_holes(rng, shape)] = np.nan
    else:
        D1[largest_at] = -SWEEP_VALUE
    return _frozen(np.zeros(shape, F32)), _frozen(D1), DISP_TOL[family]


@functools.lru_cache(maxsize=4)
def flow_case(shape, family, largest_at=None):
    """-> Uf, Vf, Ub, Vb, (a, b).  Uf = Vf = 0, so the residual of a pixel is (Ub, Vb) there (NaN where a tap of the sample is)."""
    rng = np.random.default_rng(_seed("flow", shape, family, RESEED.get(("flow", shape), 0) if family == "binades" else 0))
    if family == "integers":
        pick = rng.integers(0, len(PYTHAGOREAN), size=shape)
        table = np.array(PYTHAGOREAN, F32)
        Ub, Vb = table[pick, 0], table[pick, 1]
    else:
        Ub, Vb = _binade_values(rng, shape), np.zeros(shape, F32)
    Ub, Vb = np.asfortranarray(Ub), np.asfortranarray(Vb)
    if largest_at is None:
        Ub.reshape(-1, order="F")[_holes(rng, shape)] = np.nan
    else:
        Ub[largest_at], Vb[largest_at] = 0.0, SWEEP_VALUE
    zero = _frozen(np.zeros(shape, F32))
    return zero, zero, _frozen(Ub), _frozen(Vb), FLOW_AB[family]


# 2^53, 1, 1 in three parts of one final thread, everything else undefined or 0: (2^53 + 1) + 1 = 2^53 in ascending order, and
# 2^53 + 2 if the ones meet first.  (ncols, parts): inside the one batch of thread 0 at 3073 parts (which the binades cannot tell:
# one thread of 1024 runs it); the batch, then the tail of thread 1023; the first batch, the second, the tail of thread 0.
HAND = ((3073, (0, 1024, 2048)), (7169, (1023, 5119, 6143)), (8195, (0, 4096, 8192)))   # columns p + 1 and p + 2 must exist
HAND_BIG = 2.0 ** 53


@functools.lru_cache(maxsize=None)
def hand_case(what, ncols, parts):
    """-> the planes of disp_case (shape (1, ncols)) or flow_case ((2, ncols)): the gathered plane is NaN but for columns p and p + 1
    of the three parts, which hold 2^53, 1, 1 (first row) and 0.  The defined pixels are those of the three columns p."""
    shape = (1 if what == "disp" else 2, ncols)
    G = np.full(shape, np.nan, F32)
    for p, x in zip(parts, (HAND_BIG, 1.0, 1.0)):
        G[:, p:p + 2] = 0.0
        G[0, p] = x
    zero = _frozen(np.zeros(shape, F32))
    if what == "disp":
        return zero, _frozen(G), 1.0
    return zero, zero, _frozen(G), zero, (0.0, 1.0)


def sweep_pixel(part):
    """The pixel of SWEEP_SHAPE that carries the largest residual of part `part` (one part per column; its second row)."""
    return (1, part)


@functools.lru_cache(maxsize=4)
def cross_want(what, shape, family, largest_at=None):
    """-> (the restatement's dict of crosscheck_ref, the statistics of reduce_tree_ref on its masks and float64 magnitudes)."""
    if what == "disp":
        D0, D1, tol = disp_case(shape, family, largest_at)
        ref = cr.disp_crosscheck(D0, D1, tol)
        mag = np.abs(ref["r"])
    else:
        Uf, Vf, Ub, Vb, (a, b) = flow_case(shape, family, largest_at)
        ref = cr.flow_crosscheck(Uf, Vf, Ub, Vb, a, b)
        mag = ref["err64"]
    return ref, rt.crosscheck_stats(ref["kept_mask"], ref["defined_mask"], mag, shape[0], shape[1]), mag


@functools.lru_cache(maxsize=None)
def hand_want(what, ncols, parts):
    planes = hand_case(what, ncols, parts)
    shape = planes[0].shape
    if what == "disp":
        ref = cr.disp_crosscheck(planes[0], planes[1], planes[2])
        mag = np.abs(ref["r"])
    else:
        ref = cr.flow_crosscheck(*planes[:4], *planes[4])
        mag = ref["err64"]
    return ref, rt.crosscheck_stats(ref["kept_mask"], ref["defined_mask"], mag, shape[0], shape[1]), mag


# ---- the flow errors -------------------------------------------------------------------------------------------------------------
ERR_SIZES = (256 * ERR_TILE, 256 * ERR_TILE + 1, 512 * ERR_TILE, 512 * ERR_TILE + 1)   # 256, 257, 512, 513 tiles
ERR_PEAK_N = ERR_SIZES[3]
ERR_PEAK_TILES = (0, 255, 256, 512)
ERR_PEAK_A = 30.0   # endpoint error 2 + 30^2 = 902


def err_tiles(n):
    return (n + ERR_TILE - 1) // ERR_TILE


@functools.lru_cache(maxsize=2)   # up to a million pixels each: the tests take the cases one after the other
def error_case(n, family, masked, peak_tile=None, dead_from_tile=None):
    """-> U, V, Ut, Vt, mask (None unless masked or dead_from_tile), all (n, 1).

    integers: (u, v) = (a, 1) against (a, -1 - a^2), a = 0..4: the endpoint error is 2 + a^2 and u ut + v vt + 1 is exactly 0, so
    the angular error is acos(0) in degrees at every such pixel; a quarter of the pixels are (0, 0) against (0, 0): both errors 0.
    binades: (u, 0) against (0, 0) with |u| = m 2^e: the endpoint error is |u| itself; a few pixels are NaN.
    peak_tile: a = ERR_PEAK_A at the tile's last pixel.  dead_from_tile: the mask is 0 from that tile on."""
    rng = np.random.default_rng(_seed("err", n, family, masked, RESEED.get(("err", n, masked, dead_from_tile), 0) if family == "binades" else 0))
    shape = (n, 1)
    if family == "integers":
        a = rng.integers(0, 5, size=shape).astype(F32)
        still = rng.random(shape) < 0.25
        if peak_tile is not None:
            at = min((peak_tile + 1) * ERR_TILE, n) - 1
            a[at, 0], still[at, 0] = ERR_PEAK_A, False
        U, V = np.where(still, 0.0, a), np.where(still, 0.0, 1.0)
        Ut, Vt = U.copy(), np.where(still, 0.0, -1.0 - a * a)
    else:
        U, V = _binade_values(rng, shape), np.zeros(shape, F32)
        U[_holes(rng, shape), 0] = np.nan
        Ut, Vt = np.zeros(shape, F32), np.zeros(shape, F32)
    mask = None
    if masked or dead_from_tile is not None:
        mask = (rng.random(shape) < 0.6).astype(F32) * F32(2.0) if masked else np.ones(shape, F32)
        if dead_from_tile is not None:
            mask[dead_from_tile * ERR_TILE:, 0] = 0.0
        mask = _frozen(mask)
    return _frozen(U), _frozen(V), _frozen(Ut), _frozen(Vt), mask


def error_cases():
    """(n, family, masked, peak_tile, dead_from_tile): every size in both families with and without a mask; the largest endpoint
    error in tile 0, 255, 256 and the last; tiles 256.. all uncounted."""
    out = [(n, f, m, None, None) for n in ERR_SIZES for f in FAMILIES for m in (False, True)]
    out += [(ERR_PEAK_N, "integers", False, t, None) for t in ERR_PEAK_TILES]
    out.append((ERR_PEAK_N, "binades", False, None, 256))
    return out


def error_id(c):
    return "n%d-%s%s%s%s" % (c[0], c[1], "-masked" if c[2] else "", "" if c[3] is None else "-peak%d" % c[3], "" if c[4] is None else "-dead%d" % c[4])


@functools.lru_cache(maxsize=2)
def error_want(case):
    """-> (the restatement's dict of flowviz_ref without its compacted copies, the statistics of reduce_tree_ref on its float64
    planes)."""
    U, V, Ut, Vt, mask = error_case(*case)
    ref = fr.flow_errors(U, V, Ut, Vt, mask)
    del ref["epe64"], ref["ang64"]
    flat = lambda a: a.reshape(-1, order="F")
    return ref, rt.flow_error_stats(flat(ref["counted"]), flat(ref["epe_plane64"]), flat(ref["ang_plane64"]))


# ---- the automatic maximum ---------------------------------------------------------------------------------------------------------
PEAK = (3.0, 4.0)   # |.| = 5 exactly
ONE_STRIDE = MAXMAG_BLOCKS * BLOCK   # 262 144 threads: the scalar path's first stride in pixels, the float4 path's in float4s
MAXMAG_SCALAR = {n: (0, ONE_STRIDE - 1, ONE_STRIDE, n - 1) for n in (ONE_STRIDE, ONE_STRIDE + 1, 2 * ONE_STRIDE + 1)}
MAXMAG_VEC = {n: (4 * ONE_STRIDE - 1, 4 * ONE_STRIDE, n & ~3, n - 1) for n in (4 * ONE_STRIDE, 4 * ONE_STRIDE + 3, 4 * ONE_STRIDE + 4,
                                                                                4 * ONE_STRIDE + 7)}


def maxmag_positions(table, n):
    """The distinct positions of size n that exist (n & ~3 is n itself when there is no tail)."""
    return sorted({p for p in table[n] if 0 <= p < n})


# ---- the flat sweeps ---------------------------------------------------------------------------------------------------------------
ONE_SWEEP = FLAT_BLOCKS * BLOCK   # 1 048 576 elements: one stride of k_splat_clear and k_inpaint_merge
SPLAT_SHAPES = ((1024, 1024), (1025, 1024))
MERGE_SHAPES = ((1024, 1024), (1025, 1024), (17, 61681))   # 1 048 576, 1 049 600, 1 048 577 = 17 * 61 681 elements
