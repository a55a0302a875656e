"""A pure-Python model of the launch geometry of the fast orderings, and the case lists of the seam tests.

The red-black and zebra kernels choose their strip width from the device (occupancy x compute units), so the frames a
parity test happens to use decide where the strip seams, the ragged last strip and the row-tile edges fall -- on
one card.  The cases here FORCE the geometry through the library's per-call knobs (PDEIP_RBP_TJ, PDEIP_RB_TJ,
PDEIP_RB_SMALL, PDEIP_RB_PIPE, PDEIP_RBP_SERPENTINE, PDEIP_ALR_SMALL, PDEIP_ALR_PAIR) and carve planes at a 4-byte
offset, so the same seams are relaxed on every card.  This module needs no GPU: it restates the launch logic of
csrc/pdeip_sor_plan.hpp, pdeip_sor5.hip, pdeip_sor9.hip, pdeip_line.hip and the layouts of pdeip_sor_rbp.hpp / pdeip_sor_small.hpp (it does not
import them: a model read off the library would agree with whatever the library does) and predicts for every case the kernel
family, the kernels its launch chain really runs, their strip / tile geometry and the number of launches.
tests/test_seam_matrix.py asserts that the lists cover each coverage set; tests/test_gpu_seams.py runs them.
tests/test_sor_plan.py compares the model with the library's own plan (pdeip_debug_plan_sor, csrc/pdeip_sor_plan.hpp) on the CPU,
over the case lists and a grid of shapes; the model stays independent: it still imports nothing from the library.
"""
from collections import namedtuple

# ---- constants of the kernels -------------------------------------------------------------------------------------
RBP_S = 4                    # sweeps per pipelined launch (pdeip_sor5.hip, PS)
RBP_OWN_ROWS = 240           # pdeip_sor_rbp.hpp: 60 storing lanes x 4 rows, read as 256 with clamped halo lanes
RBP_HALO = 2 * RBP_S         # columns per side
RB_OWN_ROWS = 248            # pdeip_sor_rb.hpp: 62 storing lanes x 4 rows
RB_HALO = 4                  # rb_march2 starts three columns west of its strip and reads one more: four halo columns per side
P8_OWN_ROWS2 = 240           # pdeip_sor_pde8.hpp, the two-sweep four-colour kernel (the one-sweep kernel owns RB_OWN_ROWS)
RB_WAVES_PER_BLOCK = 4       # units per workgroup of k_sor_rb / k_pde8_colour*
PIPE_MIN_PIXELS = 1 << 21    # single-field models enter the pipeline from here on (pdeip_sor5.hip)
ALR_SMALL_MAX_PIXELS = 6144  # k_alr_small takes every frame up to here (pdeip_alr_plan.hpp)
ALR_TB_MAX = 16              # planes per transpose launch (pdeip_alr_plan.hpp)
ALR_SMALL_MAXTR = 24

# model -> (NIT iterate fields, NRO read-only fields, NCF coefficient planes)   (pdeip_models.hpp)
MODELS = {"elin4": (2, 0, 9), "llin4": (2, 2, 9), "disp4": (1, 1, 6), "dispsym4": (1, 1, 6), "pde4": (1, 0, 6), "pde8": (1, 0, 10)}
CLASS = {"elin4": "coupled", "llin4": "coupled", "disp4": "single", "dispsym4": "single", "pde4": "single", "pde8": "pde8"}
OWN = {"rbp": RBP_OWN_ROWS, "rb": RB_OWN_ROWS, "pde8": P8_OWN_ROWS2}
HALO = {"rbp": RBP_HALO, "rb": RB_HALO, "pde8": RB_HALO}
ITERS = (1, 2, 3, 4, 5, 8, 9)


def _ceil(a, b):
    return (a + b - 1) // b


# ---- RbpLayout (pdeip_sor_rbp.hpp): does the model's set of rings fit the 160 KiB of LDS? ----------------------------
def rbp_lead(model, S=RBP_S):
    """The DMA lead P that RbpLayout::pick_lead() chooses (0: none fits)."""
    nit, nro, ncf = MODELS[model]
    group, col = ncf + nro + nit, 256
    best = 0
    for p in range(1, 9):
        nk = p + 3 * (S - 1) + 1
        nq = p + 3 * (S - 1) + 1 if nro else 0
        lds = (nk * ncf * col + nq * nro * col + (p + 1) * nit * col + (S - 1) * 2 * nit * col) * 4
        if lds <= 160 * 1024 and (p - 1) * group <= 63:
            best = p
    return best


def rbp_fits(model):
    return model != "pde8" and rbp_lead(model) >= 2


def rbp_waves_per_sweep(model):
    return 2 if MODELS[model][0] == 2 else 1


# ---- SmallLayout::plan (pdeip_sor_small.hpp) ----------------------------------------------------------------------------
def small_plan(model, nrows, ncols, sweeps, qpref=1):
    """-> (ok, nslabs)"""
    nit, nro, _ = MODELS[model]
    nv = nit + nro
    vw = 4 if nv == 3 else nv
    threads, Q = (768, 5) if nv >= 4 else (1024, 4)
    if nrows < 3 or ncols < 3:
        return False, 0
    pr, hr = (nrows - 1) // 2, (nrows + 1) // 2

    def mlc(q):
        return min(threads * q // pr + 2, (152 * 1024) // (2 * hr * vw * 4))

    qq = min(qpref, Q)
    if ncols <= mlc(qq) or (ncols <= mlc(Q) and sweeps > 4):
        return True, 1
    if sweeps > 4:
        return False, 0
    H = 2 * sweeps
    for q in range(qq, Q + 1):
        w = mlc(q) - 2 * H - 1
        if w >= (H if q < Q else 4) and _ceil(ncols, w) <= 128:
            nslabs = _ceil(ncols, w)
            W = _ceil(ncols, nslabs)
            return True, _ceil(ncols, W)
    if ncols <= mlc(Q):
        return True, 1
    return False, 0


def small_launches(model, nrows, ncols, nframes, it, num_cus=256):
    """Launches of k_sor_small for the call, or None where run_sweeps does not take the small path."""
    ok, nslabs = small_plan(model, nrows, ncols, it)
    per = it
    if not ok and it > 4:
        ok, nslabs = small_plan(model, nrows, ncols, 4)
        per = 4
    if ok and nslabs > 1 and nslabs * nframes > num_cus - num_cus // 8:
        ok = False
    return _ceil(it, per) if ok else None


# ---- run_sweeps / pdeip_pde_sor8_dev: which family, how many launches ---------------------------------------------------
def family_of(model, nrows, ncols, nframes=1, it=4, small=True, pipe=True, aligned=True, num_cus=256):
    """The kernel family a red-black point-SOR call runs: 'small', 'rbp' (its 2/1 tail runs k_sor_rb), 'rb' or 'pde8'.
    A call of fewer than four sweeps never launches the pipeline (plan_chain: `n4 = pipe ? iter / 4 : 0`) and does not read
    PDEIP_RBP_TJ: it is an 'rb' call whatever the knobs allow."""
    if model == "pde8":
        return "pde8"
    if small and small_launches(model, nrows, ncols, nframes, it, num_cus) is not None:
        return "small"
    vec = nrows % 4 == 0 and aligned
    if pipe and it >= RBP_S and vec and rbp_fits(model) and (rbp_waves_per_sweep(model) == 2 or nrows * ncols >= PIPE_MIN_PIXELS):
        return "rbp"
    return "rb"


def chain(family, it):
    """Sweeps per launch of the call, in launch order."""
    out = []
    while it > 0:
        k = RBP_S if (family == "rbp" and it >= RBP_S) else (2 if it >= 2 else 1)
        out.append(k)
        it -= k
    return out


def sweep_launches(family, model, nrows, ncols, nframes, it, num_cus=256):
    """What pdeip_last_launch_count() reports after the call (the closing device-to-device copy is not counted)."""
    if it <= 0:
        return 0
    n = small_launches(model, nrows, ncols, nframes, it, num_cus) if family == "small" else len(chain(family, it))
    return 2 * n if model == "dispsym4" else n  # two independent disparity fields, one after the other


# kernel -> (rows a unit owns, halo columns per side, family whose launch chain runs it, sweeps per launch)
KERNELS = {"k_sor_rbp": (RBP_OWN_ROWS, RBP_HALO, "rbp", 4), "k_sor_rb two-sweep": (RB_OWN_ROWS, RB_HALO, "rb", 2),
           "k_sor_rb one-sweep": (RB_OWN_ROWS, 2, "rb", 1), "k_pde8_colour2": (P8_OWN_ROWS2, RB_HALO, "pde8", 2),
           "k_pde8_colour": (RB_OWN_ROWS, 2, "pde8", 1)}


def kernels_of(family, it):
    """The kernels the launch chain of the call really runs (a 'rbp' call's 2/1 tail runs k_sor_rb at the picker's width)."""
    return [k for k, (_, _, fam, sweeps) in KERNELS.items() if fam == family and sweeps in chain(family, it)]


Geometry = namedtuple("Geometry", "row_tiles last_tile_rows strips last_strip vec last_in_halo grid")


def geometry(kernel, model, nrows, ncols, tj, aligned=True):
    """Tiles and strips of one launch of `kernel` (a key of KERNELS, or a family: then its widest-halo kernel) at strip width tj."""
    kernel = {"rbp": "k_sor_rbp", "rb": "k_sor_rb two-sweep", "pde8": "k_pde8_colour2"}.get(kernel, kernel)
    own, halo, family, _ = KERNELS[kernel]
    # the marches' tiles cover rows 0 .. nrows-2; the bottom border row goes with the tile that owns the row it replicates
    # (rb_row_tiles): a frame of own + 1 rows is ONE tile.  The pipeline runs vector frames only, where that never differs.
    tiles = _ceil(nrows, own) if family == "rbp" else _ceil(nrows - 1, own)
    strips = _ceil(ncols, tj)
    last = ncols - (strips - 1) * tj
    units = tiles * strips
    grid = units if family == "rbp" else _ceil(units, RB_WAVES_PER_BLOCK)
    return Geometry(tiles, nrows - (tiles - 1) * own, strips, last, nrows % 4 == 0 and aligned, last <= halo, grid)


# ---- plan_alr (pdeip_alr_plan.hpp), restated; tests/test_alr_plan.py compares the two on the CPU ---------------------
ALR = {  # model -> (fields, distinct planes that are not the iterate, interior lines only)
    "elin4": (2, 9, False), "llin4": (2, 11, False), "llin8": (2, 15, False), "disp4": (1, 7, False), "pde4": (1, 6, False), "pde8": (1, 10, True)}


def alr_small_lds_bytes(nrows, ncols, interior):
    lo = 1 if interior else 0
    col_lines, row_lines = (ncols - 2 * lo + 1) // 2, (nrows - 2 * lo + 1) // 2
    return max(col_lines * (nrows | 1), row_lines * (ncols | 1)) * 20


def alr_family(model, nrows, ncols, small=True):
    nch, ntr, interior = ALR[model]
    if small and alr_small_lds_bytes(nrows, ncols, interior) <= 150 * 1024 and nrows * ncols <= ALR_SMALL_MAX_PIXELS and ntr <= ALR_SMALL_MAXTR:
        return "alr_small"
    return "alr_zebra"


def alr_launches(model, nrows, ncols, it, small=True, pair=True):
    """Zebra order: launches of the call.  k_alr_small: one.  Otherwise: the coefficient planes transposed (one launch per
    16), the factor planes of both directions (2), then per iteration a pass per colour along the columns, the iterate
    transposed, a pass per colour along the rows, the iterate transposed back; a coupled model relaxes both fields in one
    launch per colour (k_alr_zebra3_pair) unless PDEIP_ALR_PAIR=0.  The 9-point model runs one iteration whatever `it` is."""
    nch, ntr, interior = ALR[model]
    if model == "pde8":
        it = 1
    if it <= 0:
        return 0
    if alr_family(model, nrows, ncols, small) == "alr_small":
        return 1
    lo = 1 if interior else 0
    colours = lambda nlines: max(0, min(2, nlines - 2 * lo))
    per_colour = 1 if (pair and nch == 2) else nch
    per_iter = per_colour * colours(ncols) + 1 + per_colour * colours(nrows) + 1
    return _ceil(ntr, ALR_TB_MAX) + 2 + it * per_iter


# ---- the cases ----------------------------------------------------------------------------------------------------------
# group: A pipeline at forced widths, An widths below the picker's range, B single-field models in the pipeline, C k_sor_rb and
# the four-colour kernels at forced widths, D planes at a 4-byte offset.  family: what the case must run.  tj: forced strip
# width (None: the picker's).  serp: PDEIP_RBP_SERPENTINE.  role: which plane is carved at a one-float offset (D).
Case = namedtuple("Case", "group family model nrows ncols nframes tj it inplace col0 serp role small")


def _c(group, family, model, nrows, ncols, tj, it, inplace=True, col0=0, nframes=1, serp=0, role=None, small=False):
    return Case(group, family, model, nrows, ncols, nframes, tj, it, inplace, col0, serp, role, small)


CASES_A = [  # k_sor_rbp, coupled models: TJ in {8, 9, 16, 33, 138}, ncols = k TJ + {1, 2, 7, 8, 9, TJ-1, 0}
    _c("A", "rbp", "elin4", 4, 9, 8, 4),                                   # 2 strips, last 1; one lane of rows
    _c("A", "rbp", "llin4", 8, 18, 8, 5, inplace=False, col0=1),           # 3 strips, last 2
    _c("A", "rbp", "elin4", 236, 8, 8, 8, inplace=False),                  # 1 strip of TJ = HALO columns; own-4 rows
    _c("A", "rbp", "llin4", 240, 79, 8, 9, col0=1, serp=1),                # 10 strips (grid 10), last 7 = HALO-1 = TJ-1
    _c("A", "rbp", "elin4", 244, 26, 9, 6, serp=2),                        # 3 strips, last 8 = HALO; 2 tiles, last of 4 rows
    _c("A", "rbp", "llin4", 248, 18, 9, 7, inplace=False, serp=1),         # 2 strips, last 9 = TJ = HALO+1; last tile 8 rows
    _c("A", "rbp", "elin4", 484, 57, 16, 4, col0=1),                       # 4 strips, last 9; 3 tiles
    _c("A", "rbp", "llin4", 724, 31, 16, 4, inplace=False),                # 2 strips, last 15; 4 tiles: a grid of exactly 8
    _c("A", "rbp", "elin4", 240, 67, 33, 8, col0=1, serp=2),               # 3 strips, last 1
    _c("A", "rbp", "elin4", 8, 139, 138, 9, inplace=False, serp=1),        # 2 strips, last 1, the odd one mirrored
    # fewer than four sweeps with the pipeline allowed: k_sor_rb at the picker's width, PDEIP_RBP_TJ not read
    _c("A", "rb", "llin4", 244, 26, None, 1, inplace=False),
    _c("A", "rb", "elin4", 248, 18, None, 2, col0=1),
    _c("A", "rb", "llin4", 484, 57, None, 3),
]
CASES_A_NARROW = [  # widths the picker cannot choose (its range starts at 8)
    _c("An", "rbp", "elin4", 244, 23, 2, 8),
    _c("An", "rbp", "llin4", 8, 31, 3, 4, inplace=False, col0=1),
    _c("An", "rbp", "elin4", 484, 17, 5, 9, serp=1),
]
CASES_B = [  # single-field models at >= 2^21 pixels, and just below
    _c("B", "rbp", "disp4", 2164, 970, 970, 4),                            # 1 strip; 10 tiles, last of 4 rows
    _c("B", "rbp", "pde4", 2164, 970, 969, 8, inplace=False, col0=1),      # 2 strips, last 1
    _c("B", "rbp", "dispsym4", 2164, 970, 484, 4),                         # 3 strips, last 2
    _c("B", "rbp", "disp4", 244, 8600, 13, 8, inplace=False, serp=1),      # 662 strips, last 7; 2 tiles
    _c("B", "rbp", "pde4", 248, 8460, 16, 5, col0=1),                      # last 12; last tile 8 rows
    _c("B", "rbp", "disp4", 248, 8460, 9, 9, col0=1),                      # 940 strips of TJ = 9 = HALO+1
    _c("B", "rbp", "pde4", 240, 8744, 8, 4, inplace=False),                # 1093 strips of TJ = 8 = HALO; own rows
    _c("B", "rbp", "disp4", 4, 524288, None, 4, inplace=False),            # the picker's width, one lane of rows
    _c("B", "rbp", "pde4", 1024, 2048, 138, 8, nframes=3, inplace=False, serp=2),
    _c("B", "rbp", "disp4", 1024, 2048, None, 8),                          # 2 launches ...
    _c("B", "rb", "disp4", 1024, 2047, None, 8),                           # ... just below the switch: k_sor_rb, 4 launches
    _c("B", "rbp", "disp4", 240, 8744, 33, 6, col0=1),                     # 4 + 2; last 32 = TJ-1
    _c("B", "rbp", "pde4", 236, 8890, 16, 7, inplace=False),               # 4 + 2 + 1; own-4 rows
    _c("B", "rbp", "disp4", 236, 8890, 138, 5, serp=2),
    # fewer than four sweeps above the switch: k_sor_rb
    _c("B", "rb", "disp4", 1024, 2048, None, 1),
    _c("B", "rb", "disp4", 1024, 2048, None, 2, inplace=False, col0=1),
    _c("B", "rb", "disp4", 1024, 2048, None, 3),
]
CASES_C = [  # k_sor_rb (PDEIP_RB_PIPE=0) and k_pde8_colour / k_pde8_colour2: PDEIP_RB_TJ in {2, 3, 12, 13, 64}
    # coupled
    _c("C", "rb", "elin4", 248, 3, 2, 3),                                  # 2 strips, last 1 = TJ-1; own rows
    _c("C", "rb", "llin4", 5, 40, 2, 2, inplace=False, col0=1),            # 20 strips of TJ = 2; not vec
    _c("C", "rb", "elin4", 244, 9, 3, 5, col0=1),                          # 3 strips of TJ = 3; own-4 rows
    _c("C", "rb", "llin4", 252, 12, 12, 5, inplace=False),                 # 1 strip; 2 tiles, last of 4 rows
    _c("C", "rb", "elin4", 256, 28, 12, 9),                                # 3 strips, last 4 = HALO; last tile 8 rows
    _c("C", "rb", "llin4", 500, 29, 12, 8, col0=1),                        # last 5; 3 tiles
    _c("C", "rb", "elin4", 247, 159, 13, 4, inplace=False),                # 13 strips, last 3; not vec; grid 4
    _c("C", "rb", "llin4", 249, 38, 13, 5),                                # 3 strips, last 12 = TJ-1; one row past the tile edge
    _c("C", "rb", "elin4", 252, 642, 64, 9, inplace=False, col0=1),        # 11 strips, last 2; 22 units: grid 6
    _c("C", "rb", "llin4", 500, 450, 12, 3),                               # 38 strips, last 6... 114 units: grid 29
    _c("C", "rb", "elin4", 8, 13, 12, 1, inplace=False, col0=1),           # one sweep alone
    # single-field
    _c("C", "rb", "disp4", 248, 3, 2, 3, inplace=False),
    _c("C", "rb", "pde4", 5, 40, 2, 2, col0=1, nframes=3),
    _c("C", "rb", "dispsym4", 244, 9, 3, 5),
    _c("C", "rb", "pde4", 252, 12, 12, 5, nframes=3, inplace=False),
    _c("C", "rb", "disp4", 256, 28, 12, 9, col0=1),
    _c("C", "rb", "pde4", 500, 29, 12, 8),
    _c("C", "rb", "disp4", 247, 159, 13, 4, col0=1),
    _c("C", "rb", "dispsym4", 249, 38, 13, 5),
    _c("C", "rb", "pde4", 252, 642, 64, 9, inplace=False),
    _c("C", "rb", "disp4", 500, 450, 12, 3, inplace=False),
    _c("C", "rb", "disp4", 8, 13, 12, 1, col0=1),
    # the four-colour kernels (in place only: the entry point has no destination)
    _c("C", "pde8", "pde8", 240, 3, 2, 3),
    _c("C", "pde8", "pde8", 239, 40, 2, 2, col0=1, nframes=3),
    _c("C", "pde8", "pde8", 236, 9, 3, 3),
    _c("C", "pde8", "pde8", 244, 12, 12, 4, nframes=3),
    _c("C", "pde8", "pde8", 248, 28, 12, 5, col0=1),
    _c("C", "pde8", "pde8", 484, 29, 12, 8),
    _c("C", "pde8", "pde8", 241, 159, 13, 9, col0=1),
    _c("C", "pde8", "pde8", 244, 38, 13, 5),
    _c("C", "pde8", "pde8", 484, 642, 64, 8),
    _c("C", "pde8", "pde8", 484, 450, 12, 3, col0=1),
    _c("C", "pde8", "pde8", 249, 29, 12, 3),                               # 2 + 1 sweeps: one row past the one-sweep kernel's tile edge
    _c("C", "pde8", "pde8", 481, 29, 3, 1, nframes=3, col0=1),
    _c("C", "pde8", "pde8", 252, 12, 12, 5),                               # the one-sweep kernel's tiles are 248 rows: last of 4 rows, 1 strip
    _c("C", "pde8", "pde8", 256, 28, 12, 1, col0=1),                       # last of 8 rows
    _c("C", "pde8", "pde8", 500, 29, 12, 3),                               # 3 tiles
]
CASES_D = [  # one plane at a one-float offset, nrows % 4 == 0: the dispatch must leave the vector kernels (and the pipeline)
    _c("D", "rb", "elin4", 248, 37, None, 8, role="iterate"),
    _c("D", "rb", "elin4", 248, 37, None, 5, inplace=False, role="destination"),
    _c("D", "rb", "elin4", 484, 37, None, 9, role="coefficient", col0=1),
    _c("D", "rb", "llin4", 244, 45, None, 5, role="iterate"),              # 3 launches in place: the closing copy, unaligned
    _c("D", "rb", "llin4", 244, 45, None, 8, inplace=False, role="destination"),
    _c("D", "rb", "llin4", 244, 45, None, 4, role="coefficient"),
    _c("D", "rb", "llin4", 244, 45, None, 8, role="readonly", col0=1),
    _c("D", "rb", "disp4", 252, 51, None, 3, role="iterate"),
    _c("D", "rb", "disp4", 252, 51, None, 4, inplace=False, role="destination", col0=1),
    _c("D", "rb", "disp4", 252, 51, None, 9, role="coefficient"),
    _c("D", "rb", "disp4", 1024, 2048, None, 8, role="readonly"),          # >= 2^21 pixels: aligned, this is the pipeline (2 launches)
    _c("D", "pde8", "pde8", 244, 45, None, 5, role="iterate"),
    _c("D", "pde8", "pde8", 244, 45, None, 8, role="coefficient", nframes=3),
    _c("D", "small", "elin4", 24, 40, None, 4, role="iterate", small=True),
    _c("D", "small", "llin4", 24, 40, None, 9, role="readonly", small=True),
]
CASES = CASES_A + CASES_A_NARROW + CASES_B + CASES_C + CASES_D

# E: zebra line relaxation with k_alr_small switched off, and both sides of its 6144-pixel switch with it on
ALR_SHAPES = [(3, 3), (3, 40), (5, 300), (260, 7), (32, 48), (62, 63), (63, 64), (64, 63)]  # ALR_BLK = 63 +- 1 both ways
ALR_MODELS = ["elin4", "llin4", "llin8", "disp4", "pde4", "pde8"]
ALR_ITERS = (1, 3)
ALR_SWITCH = [(64, 96), (64, 97)]
AlrCase = namedtuple("AlrCase", "model nrows ncols nframes it small pair")


def alr_cases():
    out = []
    for model in ALR_MODELS:
        F = 3 if model == "pde4" else 1
        for shape in ALR_SHAPES:
            for it in ALR_ITERS:
                out.append(AlrCase(model, shape[0], shape[1], F, it, False, True))
                if ALR[model][0] == 2:
                    out.append(AlrCase(model, shape[0], shape[1], F, it, False, False))
        for shape in ALR_SWITCH:
            out.append(AlrCase(model, shape[0], shape[1], F, 3, True, True))
    return out


def case_id(c):
    return "-".join(str(v) for v in c)


def expected_family(c, num_cus=256):
    return family_of(c.model, c.nrows, c.ncols, c.nframes, c.it, small=c.small, pipe=c.group != "C", aligned=c.role is None, num_cus=num_cus)


def expected_launches(c, num_cus=256):
    return sweep_launches(expected_family(c, num_cus), c.model, c.nrows, c.ncols, c.nframes, c.it, num_cus)


def case_geometries(c):
    """kernel -> Geometry for the kernels the case runs AT ITS FORCED WIDTH (none: the picker's width, or the small path)."""
    if not c.tj or c.family not in OWN:
        return {}
    return {k: geometry(k, c.model, c.nrows, c.ncols, c.tj, aligned=c.role is None) for k in kernels_of(c.family, c.it)
            if c.group == "C" or k == "k_sor_rbp"}  # PDEIP_RB_TJ is set in group C only: elsewhere the marches run at the picker's width


def case_geometry(c):
    g = case_geometries(c)
    return g[next(iter(g))] if g else None


# ---- coverage -----------------------------------------------------------------------------------------------------------
def coverage_gaps(cases=None, alr=None):
    """Every value of every coverage set that the lists do NOT reach, as readable strings (empty: full coverage)."""
    cases = CASES if cases is None else cases
    alr = alr_cases() if alr is None else alr
    gaps = []

    def need(what, have, want):
        for v in want:
            if v not in have:
                gaps.append("%s: %r" % (what, v))

    for c in cases:
        if expected_family(c) != c.family:
            gaps.append("%s runs %s, not %s" % (case_id(c), expected_family(c), c.family))
        if c.family == "rbp" and c.it < RBP_S:
            gaps.append("%s: fewer than four sweeps never launch k_sor_rbp" % case_id(c))
    # Geometry counts towards a KERNEL only for the cases whose launch chain runs that kernel at the forced width.  The pipeline
    # and the two-sweep kernels (the ones that use their halo up) get the full sets; the one-sweep kernels, which run as the
    # odd tail of a call, the strip counts, the narrow last strips and the row-tile edges.
    for kernel, cls in (("k_sor_rbp", "coupled"), ("k_sor_rbp", "single"), ("k_sor_rb two-sweep", "coupled"), ("k_sor_rb two-sweep", "single"),
                        ("k_pde8_colour2", "pde8"), ("k_sor_rb one-sweep", "coupled"), ("k_sor_rb one-sweep", "single"), ("k_pde8_colour", "pde8")):
        own, halo, family, sweeps = KERNELS[kernel]
        full = sweeps > 1
        mine = [c for c in cases if c.family == family and CLASS[c.model] == cls and c.group in "ABC" and kernel in kernels_of(c.family, c.it)]
        geo = [(c, case_geometries(c)[kernel]) for c in mine if kernel in case_geometries(c)]
        tag = "%s/%s" % (kernel, cls)
        widths = set()
        for c, g in geo:
            widths.add(g.last_strip)
            if g.last_strip == c.tj - 1:
                widths.add("TJ-1")
            if g.last_strip == c.tj:
                widths.add("TJ")
        need(tag + " last-strip width", widths, [1, 2, halo - 1, halo, halo + 1, "TJ-1", "TJ"] if full else [1, 2, "TJ"])
        need(tag + " strips", {min(g.strips, 9) for _, g in geo}, [1, 2, 3, 9])
        vecs = [g for _, g in geo if g.vec]
        need(tag + " rows in the last tile", {g.last_tile_rows for g in vecs}, [4, 8, own - 4, own])
        need(tag + " row tiles", {min(g.row_tiles, 3) for _, g in geo}, [1, 2, 3])
        if family != "rbp":
            need(tag + " vec", {g.vec for _, g in geo}, [True, False])
            need(tag + " a frame one row past a tile edge", {c.nrows % own == 1 for c, g in geo}, [True])
        need(tag + " first launch of a call and a later one", {i == 0 for c in mine for i, k in enumerate(chain(c.family, c.it)) if k == sweeps}, [True, False])
        if not full:
            continue
        need(tag + " last strip inside the neighbour's halo", {g.last_in_halo for _, g in geo}, [True, False])
        need(tag + " grid >= 9 that is not a multiple of 8", {g.grid >= 9 and g.grid % 8 != 0 for _, g in geo}, [True])
        need(tag + " col0", {c.col0 for c in mine}, [0, 1])
        if family != "pde8":
            need(tag + " in place", {c.inplace for c in mine}, [True, False])
        for m in ("pde4", "pde8"):
            if any(c.model == m for c in mine):
                need(tag + " nframes of " + m, {c.nframes for c in mine if c.model == m}, [1, 3])
        need(tag + " models", {c.model for c in mine}, [m for m in MODELS if CLASS[m] == cls])
    for family, cls in (("rbp", "coupled"), ("rbp", "single"), ("rb", "coupled"), ("rb", "single"), ("pde8", "pde8")):
        mine = [c for c in cases if c.family == family and CLASS[c.model] == cls and c.group in "ABC"]
        # every launch chain and both ping-pong parities; the pipeline's chains start at four sweeps (4, 4+1, 4+2, 4+2+1, 4+4, 4+4+1)
        need("%s/%s iter" % (family, cls), {c.it for c in mine}, (4, 5, 6, 7, 8, 9) if family == "rbp" else ITERS)
    for cls in ("coupled", "single"):  # calls too short for the pipeline, with the pipeline allowed
        need("%s iter below four with the pipeline on" % cls,
             {c.it for c in cases if c.group in "AB" and CLASS[c.model] == cls and c.family == "rb" and c.nrows % 4 == 0 and c.it < RBP_S}, [1, 2, 3])
    a = [c for c in cases if c.group == "A"]
    need("A forced widths", {c.tj for c in a}, [8, 9, 16, 33, 138])
    need("A serpentine modes", {c.serp for c in a}, [0, 1, 2])
    need("A row counts", {c.nrows for c in a}, [4, 8, 236, 240, 244, 248, 484, 724])
    need("An widths below the picker's range", {c.tj for c in cases if c.group == "An"}, [2, 3, 5])
    b = [c for c in cases if c.group == "B"]
    need("B frames", {(c.nrows, c.ncols) for c in b}, [(4, 524288), (244, 8600), (2164, 970), (1024, 2048), (1024, 2047)])
    need("B both sides of the 2^21 switch", {(c.family, c.nrows * c.ncols >= PIPE_MIN_PIXELS) for c in b}, [("rbp", True), ("rb", False)])
    need("B pde4 with three frames in the pipeline", {(c.model, c.nframes, c.family) for c in b}, [("pde4", 3, "rbp")])
    need("B models with a forced width", {c.model for c in b if c.tj}, ["disp4", "pde4", "dispsym4"])
    need("B iter", {c.it for c in b if c.family == "rbp"}, [4, 8])
    need("B one model and iter on both sides of the switch, with different launch counts",
         {True for x in b for y in b if (x.model, x.it, x.nrows) == (y.model, y.it, y.nrows) and x.family == "rbp" and y.family == "rb"
          and expected_launches(x) != expected_launches(y)}, [True])
    cc = [c for c in cases if c.group == "C"]
    need("C forced widths", {c.tj for c in cc}, [2, 3, 12, 13, 64])
    need("C k_sor_rb rows", {c.nrows for c in cc if c.family == "rb"}, [5, 247, 248, 249, 252, 500])
    need("C pde8 rows", {c.nrows for c in cc if c.family == "pde8"}, [239, 240, 241, 244, 484, 249])
    need("C iter", {c.it for c in cc}, [1, 2, 3, 5])
    d = [c for c in cases if c.group == "D"]
    for c in d:
        if c.nrows % 4:
            gaps.append("D %s: nrows must be a multiple of 4" % case_id(c))
    need("D roles", {c.role for c in d}, ["iterate", "destination", "coefficient", "readonly"])
    need("D model x role", {(c.model, c.role) for c in d},
         [(m, r) for m in ("elin4", "llin4", "disp4", "pde8") for r in ("iterate", "destination", "coefficient", "readonly")
          if not (r == "readonly" and MODELS[m][1] == 0) and not (r == "destination" and m == "pde8")])
    need("D a small frame with the small path on", {c.family for c in d}, ["small"])
    # an aligned twin of the case would have run another chain: the launch count shows that the dispatch noticed
    need("D a case whose launch count differs from its aligned twin's",
         {expected_launches(c) != sweep_launches(family_of(c.model, c.nrows, c.ncols, c.nframes, c.it, small=c.small), c.model, c.nrows,
                                                 c.ncols, c.nframes, c.it) for c in d}, [True])
    for model in ALR_MODELS:
        mine = [c for c in alr if c.model == model]
        need("E %s shapes without k_alr_small" % model, {(c.nrows, c.ncols) for c in mine if not c.small}, ALR_SHAPES)
        need("E %s iter" % model, {c.it for c in mine if not c.small}, ALR_ITERS)
        need("E %s sides of the 6144-pixel switch" % model, {alr_family(c.model, c.nrows, c.ncols, c.small) for c in mine if c.small}, ["alr_small", "alr_zebra"])
        if ALR[model][0] == 2:
            need("E %s pair" % model, {c.pair for c in mine if not c.small}, [True, False])
        if model == "pde4":
            need("E pde4 frames", {c.nframes for c in mine}, [3])
    return gaps


# ---- the range-laced cases (tests/range_problems.py) --------------------------------------------------------------------------
# The same families, forced by the same knobs, on problems whose divisors leave the range of ordinary numbers; run by
# tests/test_gpu_range.py, and on the CPU (finite share, census, wave mix) by tests/test_range_problems.py.  A RangeCase wraps a
# Case -- its group letter keeps its meaning for the knobs: A / B the pipeline, C the marches with PDEIP_RB_PIPE=0, D here the small
# path with the knobs at their defaults -- and adds the relaxation factor and the lacing.  div_frac is the share of EACH of the three
# out-of-range divisor classes: 0.002 leaves clean waves next to fallback waves in one launch of k_sor_rbp, 0 none that falls
# back, 0.1 none that stays clean.
RangeCase = namedtuple("RangeCase", "case omega frac div_frac corner")
RANGE_SEED = 4200
RANGE_OMEGA = {"elin4": 1.9, "llin4": 1.9, "llin8": 1.9, "disp4": 1.9, "dispsym4": 1.9, "pde4": 1.75, "pde8": 1.75}
RANGE_MIXED, RANGE_CLEAN, RANGE_FALLBACK = 0.002, 0.0, 0.1
# The cases that go through a gateway (exact order, line relaxation) compare the residual outputs too, and a residual is infinite
# wherever the divisor data is: at the default share of 1 % per class the residual planes of the flow gateways are 98.99 % finite,
# short of the 99 % every output plane of every case has to keep.  0.4 % per out-of-range divisor class leaves them above 99.5 %.
RANGE_GATEWAY_DIV = 0.004
from range_problems import CORNER_MIN_PIXELS  # class T: point SOR only, from this frame size on


def corner_fits(model, nrows, ncols, it):
    """Class T in colour order: a sweep is two half-sweeps (four quarter-sweeps of the 9-point model), and each carries a non-finite
    value one pixel further, so after `it` sweeps the pixels within k it of the class's pixel can be non-finite, k = 2 (4) -- at most
    (k it + 1)^2 of them inside the frame.  The case gets the class only where that is within the 1 % of a plane that may be
    non-finite (and the frame has the 8192 pixels)."""
    k = 4 if model == "pde8" else 2
    return nrows * ncols >= max(CORNER_MIN_PIXELS, 100 * (k * it + 1) ** 2)


def _r(case, omega, div_frac=None, frac=0.01):
    # class T wherever the frame is large enough for it, but not where no wave is to fall back: its denominator is subnormal
    return RangeCase(case, omega, frac, div_frac, corner_fits(case.model, case.nrows, case.ncols, case.it) and div_frac != RANGE_CLEAN)


def _range_small():  # k_sor_small, knobs at their defaults: (37, 53) and (131, 70), iter 4 and 9
    out = []
    for mi, model in enumerate(("elin4", "llin4", "disp4", "dispsym4", "pde4")):
        for si, (nrows, ncols) in enumerate(((37, 53), (131, 70))):
            for ii, it in enumerate((4, 9)):
                k = mi + si + ii
                inplace = model == "dispsym4" or k % 2 == 0
                out.append(_r(_c("D", "small", model, nrows, ncols, None, it, inplace=inplace, col0=(mi + ii) % 2, small=True),
                              (1.0, RANGE_OMEGA[model])[(mi + si) % 2]))
    return out


def _range_rb():  # k_sor_rb and the four-colour kernels: PDEIP_RB_TJ in {3, 13}, iter 1, 2, 3 (one- and two-sweep kernels, first and later launches)
    out = []
    for mi, model in enumerate(("elin4", "llin4", "disp4", "dispsym4", "pde4", "pde8")):
        for si, (nrows, ncols) in enumerate(((252, 51), (8, 139))):
            for ii, it in enumerate((1, 2, 3)):
                inplace = model in ("dispsym4", "pde8") or (mi + si) % 2 == 0
                out.append(_r(_c("C", "pde8" if model == "pde8" else "rb", model, nrows, ncols, (3, 13)[(mi + si + ii) % 2], it, inplace=inplace,
                                 col0=(si + ii) % 2), (1.0, RANGE_OMEGA[model])[(mi + ii) % 2]))
    return out


def _range_rbp():
    out = []
    # coupled models, clean waves beside fallback waves: TJ in {9, 33}, iter 4 and 9 (4 + 4 + 1), every serpentine mode, in place and _to, both col0
    k = 0
    for model in ("elin4", "llin4"):
        for nrows, ncols in ((244, 300), (484, 57)):
            for tj in (9, 33):
                for it in (4, 9):
                    out.append(_r(_c("A", "rbp", model, nrows, ncols, tj, it, inplace=(k // 3) % 2 == 0, col0=(k // 2) % 2, serp=k % 3),
                                  (1.0, RANGE_OMEGA[model])[(k // 4 + k) % 2], RANGE_MIXED))
                    k += 1
    # single-field models at the 2^21 switch, one forced width each; disp4 also mirrored: its derive() is not symmetric in wW / wE
    out += [_r(_c("B", "rbp", "disp4", 1024, 2048, 138, 4), 1.0, RANGE_MIXED),
            _r(_c("B", "rbp", "disp4", 1024, 2048, 33, 9, inplace=False, col0=1, serp=1), 1.9, RANGE_MIXED),
            _r(_c("B", "rbp", "disp4", 1024, 2048, 138, 4, serp=1), 1.0, RANGE_MIXED),
            _r(_c("B", "rbp", "pde4", 1024, 2048, 138, 8, nframes=3, inplace=False, serp=2), 1.0, RANGE_MIXED),
            _r(_c("B", "rbp", "dispsym4", 1024, 2048, 484, 4, col0=1), 1.0, RANGE_MIXED)]
    # every wave clean, every wave falling back: with the mixed cases, the three outcomes of the ballot
    for model in ("elin4", "llin4"):
        out += [_r(_c("A", "rbp", model, 240, 67, 33, 4, col0=1, serp=2), 1.0, RANGE_CLEAN),
                _r(_c("A", "rbp", model, 240, 67, 33, 5, inplace=False, serp=1), 1.0, RANGE_FALLBACK)]
    for model in ("disp4", "pde4", "dispsym4"):
        out += [_r(_c("B", "rbp", model, 1024, 2048, 138, 4), 1.0, RANGE_CLEAN),
                _r(_c("B", "rbp", model, 1024, 2048, 138, 4, col0=1, serp=0 if model == "dispsym4" else 1), 1.0, RANGE_FALLBACK)]
    return out


RANGE_SMALL, RANGE_RB, RANGE_RBP = _range_small(), _range_rb(), _range_rbp()
RANGE_CASES = RANGE_SMALL + RANGE_RB + RANGE_RBP


def range_case_id(rc):
    return "%s-w%g-d%s" % (case_id(rc.case), rc.omega, rc.div_frac)


# Exact order, solver 1, through the gateways: every form of the wavefront kernels.  form -> the knobs that force it.
EXACT_FORMS = {"persist": dict(PDEIP_EXACT_PERSIST=1, PDEIP_EXACT_WALK=0, PDEIP_PDE8_PERSIST=1), "front": dict(PDEIP_EXACT_PERSIST=0, PDEIP_PDE8_PERSIST=0),
               "walk": dict(PDEIP_EXACT_PERSIST=1, PDEIP_EXACT_WALK=1)}
RANGE_EXACT_MODELS = ("elin4", "llin4", "llin8", "disp4", "dispsym4", "pde4", "pde8")
RANGE_EXACT_FRAMES = ((37, 53), (131, 70), (244, 300))
RANGE_EXACT_OMEGAS, RANGE_EXACT_ITERS = (1.0, 1.9), (1, 4)
ExactCase = namedtuple("ExactCase", "model nrows ncols nframes it omega corner")


def exact_forms(model):
    return ("persist", "front") if model == "pde8" else ("persist", "front", "walk")  # the 9-point walker has one persistent form


def range_exact_cases(model):
    return [ExactCase(model, r, c, 2 if model in ("pde4", "pde8") and (r, c) == (37, 53) else 1, it, om, r * c >= CORNER_MIN_PIXELS)
            for r, c in RANGE_EXACT_FRAMES for om in RANGE_EXACT_OMEGAS for it in RANGE_EXACT_ITERS]


def exact_launches(model, nrows, ncols, it, form):
    """pdeip_last_launch_count() after an exact-order point-SOR call (run_sweeps, pdeip_pde_sor8_dev): the persistent forms make
    three launches (pack the coefficients, walk, fill the borders); the launch-per-front form derives, then makes one launch per
    front m = a + G b + H t of (row tiles of 64 steps) x (strips of 64 columns) x sweeps, then fills the borders."""
    if it <= 0:
        return 0
    if form != "front":
        n = 3
    else:
        skew, g, h = (2, 3, 4) if model == "pde8" else (1, 2, 3)
        a, b = (nrows - 2 + skew * 63 + 63) // 64, (ncols - 2 + 63) // 64
        n = 1 + ((a - 1) + g * (b - 1) + h * (it - 1) + 1) + 1
    return 2 * n if model == "dispsym4" else n


def alr_exact_launches(model, nrows, ncols, it):
    """Exact order: launches of a line-relaxation call (plan_alr).  The coefficient planes transposed (one launch per
    16), the factor planes of both directions (2), then per iteration a pass along the columns, the iterate transposed, a pass
    along the rows, the iterate transposed back.  A pass of a coupled model walks both chains in one launch (k_alr_lex<2>) where two
    lines of float4 fit the 160 KiB of LDS, and one chain per launch otherwise -- which is how a call shows the form it ran."""
    nch, ntr, _ = ALR[model]
    if model == "pde8":
        it = 1
    if it <= 0:
        return 0
    one_pass = lambda n: 1 if nch == 2 and 2 * 16 * n <= 160 * 1024 else nch
    return _ceil(ntr, ALR_TB_MAX) + 2 + it * (one_pass(nrows) + 1 + one_pass(ncols) + 1)


# Line relaxation, solver 2, no class T.  Exact order: pair and single chain (a line of 5200 elements holds one chain at a time).
# Zebra: k_alr_small on (37, 53); k_alr_zebra3 / k_alr_zebra3_pair on (131, 70) and (226, 450) with PDEIP_ALR_SMALL=0, PDEIP_ALR_PAIR 0 / unset.
RANGE_ALR_OMEGAS, RANGE_ALR_ITERS = (1.0, 1.4), (1, 3)
RANGE_ALR_EXACT_FRAMES = ((37, 53), (131, 70), (7, 5200))
RANGE_ALR_ZEBRA_FRAMES = ((37, 53, True), (131, 70, False), (226, 450, False))  # (nrows, ncols, k_alr_small allowed)
AlrRangeCase = namedtuple("AlrRangeCase", "model nrows ncols nframes it omega zebra small pair")


def range_alr_cases(model):
    out = []
    F = lambda r, c: 2 if model in ("pde4", "pde8") and (r, c) == (37, 53) else 1
    for om in RANGE_ALR_OMEGAS:
        for it in RANGE_ALR_ITERS:
            for r, c in RANGE_ALR_EXACT_FRAMES:
                out.append(AlrRangeCase(model, r, c, F(r, c), it, om, False, True, True))
            for r, c, small in RANGE_ALR_ZEBRA_FRAMES:
                out.append(AlrRangeCase(model, r, c, F(r, c), it, om, True, small, True))
                if not small and ALR[model][0] == 2:
                    out.append(AlrRangeCase(model, r, c, F(r, c), it, om, True, small, False))
    return out
