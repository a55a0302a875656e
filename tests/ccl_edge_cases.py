"""More masks for the connected-component tests, chosen from the kernels' own constants (csrc/pdeip_ccl_plan.hpp) and not from
topology: planes at and just past the one-workgroup form's limit, vertical runs that start and end at known places of the 64-row
chunks, every pattern around a four-tile corner and astride a tile seam, planes of 256 / 257 / 512 / 513 blocks for the scan,
ties on the far side of the argmax's stride, and label sets that collide and wrap in the area table of k_ccl_relabel.  The same
(name, A) interface as ccl_cases.py; tests/test_ccl_edge_cases.py proves that each case is what it claims.  Planes are built
once per process and are read-only."""
import functools

import numpy as np

import ccl_cases
from ccl_cases import SMALL_MAX_PIX, _f

TILE_I, TILE_J = 64, 32  # pdeip_ccl_plan.hpp

SMALL_LIMIT_SHAPES = ((128, 128), (16384, 1), (1, 16384), (4096, 4), (4, 4096), (127, 129), (129, 127))
PAST_LIMIT_SHAPE = (5, 3277)  # 16 385 pixels
PATTERN_SHAPE_2 = (126, 130)  # two chunks per column, 16 380 pixels
PATTERN_SHAPE_4 = (200, 80)   # four chunks per column, the two in the middle whole
CARRY_ROWS = 260
CARRY_ENDS = (0, 1, 62, 63, 64, 65, 126, 127, 128, 129, 191, 192, 193, 255, 256, 259)
CARRY_PAIRS = tuple((a, b) for a in CARRY_ENDS for b in CARRY_ENDS if a <= b)  # 136
CARRY_RUNS_PER_PLANE = 32  # 260 x 63 = 16 380 pixels
SEAM_ROWS, SEAM_COLS = (63, 64, 65, 128, 129), (31, 32, 33, 64, 65)
CORNER_SHAPE = (330, 170)  # 6 x 6 tiles: 5 x 5 inner four-tile corners
SCAN_SHAPES = {256: (512, 512), 257: (513, 512), 512: (1024, 512), 513: (1026, 512)}  # blocks of LIN_PIX pixels: plane
RAKE_SHAPES = ((256, 300), (512, 512))
WRAP_SHAPE = (64, 480)
WRAP_LINE_LABELS = (987, 1597)  # hash to slot 2047 and to slot 0


def alternating(shape):
    """Every second pixel in memory (column-major) order."""
    return (np.arange(shape[0] * shape[1]) % 2 == 0).reshape(shape[1], shape[0]).T


def carry_plane(pairs):
    """One vertical run [a, b] per pair, in the columns 0, 2, 4, ...: component k + 1 is run k and has b - a + 1 pixels."""
    m = np.zeros((CARRY_ROWS, 2 * len(pairs) - 1), bool)
    for k, (a, b) in enumerate(pairs):
        m[a:b + 1, 2 * k] = True
    return m


def corner_places(shape=CORNER_SHAPE):
    """(i0, j0) of every inner four-tile corner: pixel (i0, j0) is the first of its tile."""
    return [(i0, j0) for i0 in range(TILE_I, shape[0], TILE_I) for j0 in range(TILE_J, shape[1], TILE_J)]


CORNER_PIXELS = ((-1, -1), (-1, 0), (0, -1), (0, 0))  # bit k of a pattern switches pixel (i0 + di, j0 + dj) on


def corner_plane(arms):
    """Pattern k % 16 of the 2 x 2 pixels around corner k, nothing else; with arms every such pixel is the end of a three-pixel
    diagonal that runs away from the corner inside its own tile, so that under conn 8 the tile roots are not the corner pixels."""
    m = np.zeros(CORNER_SHAPE, bool)
    for k, (i0, j0) in enumerate(corner_places()):
        for bit, (di, dj) in enumerate(CORNER_PIXELS):
            if (k % 16) >> bit & 1:
                si, sj = (-1 if di < 0 else 1), (-1 if dj < 0 else 1)
                for t in range(3 if arms else 1):
                    m[i0 + di + si * t, j0 + dj + sj * t] = True
    return m


def _clear_of(seams, lo, hi, step):
    """Centres lo, lo + step, ... below hi that keep three pixels away from every seam."""
    return [c for c in range(lo, hi, step) if all(abs(c - s) > 3 for s in seams)]


SEAM_WEST = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0))  # NW, W, SW, N, S of a pixel in column 32
SEAM_NORTH = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1))  # NW, N, NE, W, E of a pixel in row 64


def seam_pattern_places(kind):
    """(shape, centres): the 32 pixels that carry the 32 patterns, on column 32 (kind 'col') or on row 64 (kind 'row')."""
    if kind == "col":
        shape = (200, 40)
        rows = _clear_of(range(TILE_I, shape[0], TILE_I), 2, shape[0] - 2, 5)[:32]
        return shape, [(i, TILE_J) for i in rows]
    shape = (70, 200)
    cols = _clear_of(range(TILE_J, shape[1], TILE_J), 2, shape[1] - 2, 5)[:32]
    return shape, [(TILE_I, j) for j in cols]


def seam_pattern_plane(kind):
    """Every on/off pattern of the five neighbours that west_rules (column seam) or the row-seam half of k_ccl_seam reads, each
    around its own foreground pixel on the seam, away from the corners."""
    shape, places = seam_pattern_places(kind)
    m = np.zeros(shape, bool)
    for k, (i, j) in enumerate(places):
        m[i, j] = True
        for bit, (di, dj) in enumerate(SEAM_WEST if kind == "col" else SEAM_NORTH):
            if k >> bit & 1:
                m[i + di, j + dj] = True
    return m


def lattice(shape):
    """Isolated pixels with period 4, and the first and the last pixel of the plane."""
    ii, jj = np.indices(shape)
    m = (ii % 4 == 0) & (jj % 4 == 0)
    m[0, 0] = m[-1, -1] = True
    return m


def singletons_with_triples(n, triples):
    """n x n, isolated pixels with period 2: pixel (2a, 2b) is component b * n/2 + a + 1.  Each (a, b) of triples joins (2a, 2b)
    with the pixel two rows below it, which takes one label out of the sequence and leaves a component of three pixels."""
    ii, jj = np.indices((n, n))
    m = (ii % 2 == 0) & (jj % 2 == 0)
    for a, b in triples:
        m[2 * a + 1, 2 * b] = True
    return m


def rake(shape, seed):
    """A line on every fourth row from a random column to the last one; isolated pixels on the rows half way between, which use
    up label numbers, so that a block of 1024 pixels meets the labels of lines that started far apart."""
    rng = np.random.default_rng(seed)
    rows, cols = shape
    m = np.zeros(shape, bool)
    for i in range(0, rows, 4):
        m[i, rng.integers(0, cols):] = True
    m[2::4, 0::2] = rng.random(m[2::4, 0::2].shape) < 0.8
    return m


def wrap_plane():
    """64 rows, so a block of 1024 pixels is 16 columns.  Isolated pixels on the even rows 2..60 of every second column; a line
    on row 0 and one on row 63, each to the last column, started where they become the components 987 (slot 2047 of the area
    table) and 1597 (slot 0); the last column of isolated pixels before each line is cut short to make the count come out.  Every later
    block holds both lines; the ones in which an isolated pixel is component 2584, 5168 or 6765 (slot 2047 again) make the probe
    wrap from slot 2047 to slot 0 and find it taken."""
    rows, cols = WRAP_SHAPE
    m = np.zeros(WRAP_SHAPE, bool)
    per_col = len(range(2, 61, 2))
    count, j, starts = 0, 0, []
    for want, row in zip(WRAP_LINE_LABELS, (0, rows - 1)):
        while want - 1 - count >= per_col:
            m[2:61:2, j] = True
            count += per_col
            j += 2
        m[2:2 + 2 * (want - 1 - count):2, j] = True  # a partial column, possibly empty
        count = want
        m[row, j + 1:] = True
        starts.append(j + 1)
        j += 2
    m[2:61:2, j::2] = True
    return m, tuple(starts)


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, mask):
        a = _f(mask)
        a.setflags(write=False)
        out.append((name, a))

    # a. the limits of the one-workgroup form
    for k, shape in enumerate(SMALL_LIMIT_SHAPES):
        rng = np.random.default_rng(4000 + k)
        add("small_%dx%d_fg" % shape, np.ones(shape))
        add("small_%dx%d_r50" % shape, rng.random(shape) < 0.5)
        add("small_%dx%d_alt" % shape, alternating(shape))
    ii, jj = np.indices((128, 128))
    add("small_128x128_checker", (ii + jj) % 2 == 0)
    add("past_%dx%d_r50" % PAST_LIMIT_SHAPE, np.random.default_rng(4100).random(PAST_LIMIT_SHAPE) < 0.5)
    r, c = PATTERN_SHAPE_2
    ii, jj = np.indices(PATTERN_SHAPE_2)
    add("serpentine_%dx%d" % (r, c), ccl_cases.serpentine(r, c))
    add("spiral_%dx%d" % (r, c), ccl_cases.spiral(r, c))
    for spine in ("last_row", "first_row", "last_col", "first_col"):
        add("comb_%s_%dx%d" % (spine, r, c), ccl_cases.comb(r, c, spine))
    add("diag_plus_%dx%d" % (r, c), (ii + jj) % 4 == 0)
    add("diag_minus_%dx%d" % (r, c), (ii - jj) % 4 == 0)
    r, c = PATTERN_SHAPE_4
    add("serpentine_%dx%d" % (r, c), ccl_cases.serpentine(r, c))
    for spine in ("last_row", "first_row"):
        add("comb_%s_%dx%d" % (spine, r, c), ccl_cases.comb(r, c, spine))
    for k in range(0, len(CARRY_PAIRS), CARRY_RUNS_PER_PLANE):
        add("carry_%d" % (k // CARRY_RUNS_PER_PLANE), carry_plane(CARRY_PAIRS[k:k + CARRY_RUNS_PER_PLANE]))
    add("carry_all", carry_plane(CARRY_PAIRS))
    # b. tile seams and corners
    for a, rows in enumerate(SEAM_ROWS):
        for b, cols in enumerate(SEAM_COLS):
            add("seam_%dx%d_r50" % (rows, cols), np.random.default_rng(5000 + 10 * a + b).random((rows, cols)) < 0.5)
            add("seam_%dx%d_fg" % (rows, cols), np.ones((rows, cols)))
    add("corners_%dx%d" % CORNER_SHAPE, corner_plane(False))
    add("corner_arms_%dx%d" % CORNER_SHAPE, corner_plane(True))
    add("seam_patterns_col32", seam_pattern_plane("col"))
    add("seam_patterns_row64", seam_pattern_plane("row"))
    # c. the rounds of the scan and the far side of the argmax
    for blocks, shape in SCAN_SHAPES.items():
        add("lattice_%dx%d_%dblocks" % (shape + (blocks,)), lattice(shape))
    add("largest_far_tie_80x80", singletons_with_triples(80, ((3, 1), (10, 30))))      # components 44 and 1210, three pixels each
    add("largest_far_unique_80x80", singletons_with_triples(80, ((20, 35),)))          # component 1421
    add("largest_far_tie_160x160", singletons_with_triples(160, ((5, 2), (40, 60))))   # components 166 and 4840
    add("largest_far_unique_160x160", singletons_with_triples(160, ((7, 70),)))        # component 5608
    # d. the area table
    for k, shape in enumerate(RAKE_SHAPES):
        add("rake_%dx%d" % shape, rake(shape, 6000 + k))
    add("wrap_%dx%d" % WRAP_SHAPE, wrap_plane()[0])
    return tuple(out)


def names():
    return [n for n, _ in cases()]


def get(name):
    return dict(cases())[name]


def admits_small(A):
    return A.size <= SMALL_MAX_PIX
