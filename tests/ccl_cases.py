"""The masks of the connected-component tests, each chosen for a way a parallel labelling can go wrong.  A case is (name, A) with A
float32 [rows, cols]; every case is run with conn 4 and 8 and, on the GPU, in both forms wherever the small one admits the size.
Planes are built once per process and never modified."""
import functools

import numpy as np

SMALL_MAX_PIX = 16384  # pdeip_ccl_plan.hpp: the largest plane the one-workgroup form admits
RANDOM_SIZES = ((17, 33), (63, 65), (130, 67), (257, 129), (511, 769))
RANDOM_DENSITIES = (0.3, 0.5, 0.6, 0.9)
CLASSES = ("min", "random", "checker", "diag", "serpentine", "spiral", "comb", "threshold", "largest")


def _f(mask):
    return np.ascontiguousarray(np.asarray(mask, dtype=np.float32))


def serpentine(rows, cols):
    """One pixel wide: every second column is full, joined to the next one alternately at the bottom and at the top."""
    m = np.zeros((rows, cols), bool)
    m[:, 0::2] = True
    for k, j in enumerate(range(1, cols, 2)):
        m[rows - 1 if k % 2 == 0 else 0, j] = True
    return m


def spiral(rows, cols):
    """One pixel wide square spiral from the corner (0, 0) inwards, a free pixel between the windings: the walk turns right
    whenever the pixel two ahead is taken or the border is reached."""
    m = np.zeros((rows, cols), bool)
    i, j, di, dj = 0, 0, 0, 1
    m[0, 0] = True
    while True:
        moved = False
        while True:
            a, b, c, d = i + di, j + dj, i + 2 * di, j + 2 * dj
            if not (0 <= a < rows and 0 <= b < cols) or m[a, b] or (0 <= c < rows and 0 <= d < cols and m[c, d]):
                break
            i, j = a, b
            m[i, j] = True
            moved = True
        if not moved:
            return m
        di, dj = dj, -di


def comb(rows, cols, spine):
    m = np.zeros((rows, cols), bool)
    if spine in ("last_row", "first_row"):
        m[:, 0::2] = True
        m[rows - 1 if spine == "last_row" else 0, :] = True
    else:
        m[0::2, :] = True
        m[:, cols - 1 if spine == "last_col" else 0] = True
    return m


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for shape in ((1, 1), (1, 70), (70, 1), (2, 2)):
        n = shape[0] * shape[1]
        out.append(("min_%dx%d_fg" % shape, _f(np.ones(shape))))
        out.append(("min_%dx%d_bg" % shape, _f(np.zeros(shape))))
        out.append(("min_%dx%d_alt" % shape, _f((np.arange(n) % 2 == 0).reshape(shape[1], shape[0]).T)))
    for k, shape in enumerate(RANDOM_SIZES):
        for d in RANDOM_DENSITIES:
            rng = np.random.default_rng(1000 * k + int(100 * d))
            out.append(("random_%dx%d_%02d" % (shape + (int(100 * d),)), _f(rng.random(shape) < d)))
    ii, jj = np.indices((64, 64))
    out.append(("checker_64x64", _f((ii + jj) % 2 == 0)))
    ii, jj = np.indices((130, 131))
    out.append(("diag_plus_130x131", _f((ii + jj) % 4 == 0)))
    out.append(("diag_minus_130x131", _f((ii - jj) % 4 == 0)))
    out.append(("serpentine_130x131", _f(serpentine(130, 131))))
    out.append(("spiral_130x131", _f(spiral(130, 131))))
    for spine in ("last_row", "first_row", "last_col", "first_col"):
        out.append(("comb_%s_130x131" % spine, _f(comb(130, 131, spine))))
    rng = np.random.default_rng(77)
    t = rng.random((67, 130)).astype(np.float32) - np.float32(0.45)
    special = np.array([np.nan, 0.0, -0.0, -np.inf, np.inf, 1e-45, -1e-45], np.float32)
    t.flat[rng.choice(t.size, 7 * 200, replace=False)] = np.tile(special, 200)
    out.append(("threshold_67x130", t))
    # largest component: a tie (the lower label wins), the largest as the last label, no foreground
    tie = np.zeros((40, 90), np.float32)
    tie[3:9, 2:7] = 1.0
    tie[20:25, 60:66] = 2.0  # 30 pixels each
    tie[30, 30] = 1.0
    out.append(("largest_tie_40x90", tie))
    last = np.zeros((70, 140), np.float32)
    last[1, 1] = last[5:7, 5] = 1.0
    last[10:60, 100:139] = 3.0
    out.append(("largest_last_70x140", last))
    out.append(("largest_none_70x140", -np.ones((70, 140), np.float32)))
    return tuple(out)


def names():
    return [n for n, _ in cases()]


def get(name):
    """A case of this list or of ccl_edge_cases.py (which imports this module, hence the late import)."""
    own = dict(cases())
    if name in own:
        return own[name]
    import ccl_edge_cases

    return ccl_edge_cases.get(name)


def admits_small(A):
    return A.size <= SMALL_MAX_PIX
