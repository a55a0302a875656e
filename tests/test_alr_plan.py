"""CPU: the library's own launch plan of a line-relaxation call (pdeip_debug_plan_alr, csrc/pdeip_alr_plan.hpp) against the
independent models that already exist -- seam_model.alr_launches / alr_exact_launches and line_scan_cases.scan_launches -- under the
knobs, over a grid of shapes that holds every boundary of the decision +-1; then family, kernel, chains per launch, G, LDS bytes,
colours and workspace at those boundaries, stated by hand.  The entry makes no HIP call."""
import itertools

import pytest

import line_scan_cases as lsc
import seam_model as sm
from alr_plan import EXACT, LINE_SCAN, RED_BLACK, plan_alr
from sor_plan import knobs

KIB = 1024
# the minimum frame; the 6144-pixel gate of k_alr_small both ways round; ordinary frames; lines at every boundary of the scan tree
# (2048 / 4096 coupled, 4096 / 8192 single-field: G 1 -> 2 -> 3), of the exact-order rules (5120: two chains of float4 in 160 KiB,
# 10240: one) and one past the third group of a coupled scan (6145), each +1, the short side 3 to 6
LONG = (2048, 2049, 4096, 4097, 5120, 5121, 6145, 8192, 8193, 10240, 10241)
SHAPES = ([(3, 3), (3, 2048), (3, 2049), (2048, 3), (2049, 3), (4, 5), (64, 96), (64, 97)]
          + [s for k, n in enumerate(LONG) for s in ((n, 3 + k % 4), (3 + (k + 1) % 4, n))])
ITERS = (1, 3)


@pytest.fixture(scope="module")
def capi(pdeip):
    return pdeip.capi


@pytest.mark.parametrize("model", sm.ALR_MODELS)
def test_launch_counts_over_a_grid_of_shapes(capi, model):
    for (nrows, ncols), it in itertools.product(SHAPES, ITERS):
        what = (model, nrows, ncols, it)
        for small, pair in itertools.product((True, False), repeat=2):
            with knobs(PDEIP_ALR_SMALL=None if small else 0, PDEIP_ALR_PAIR=None if pair else 0):
                p = plan_alr(capi, model, nrows, ncols, 1, it, RED_BLACK)
            assert p.nlaunch == sm.alr_launches(model, nrows, ncols, it, small=small, pair=pair), what + (small, pair)
            assert p.family == ("small" if sm.alr_family(model, nrows, ncols, small) == "alr_small" else "zebra"), what + (small, pair)
        with knobs():
            exact, scan = plan_alr(capi, model, nrows, ncols, 1, it, EXACT), plan_alr(capi, model, nrows, ncols, 1, it, LINE_SCAN)
        with knobs(PDEIP_ALR_SCAN=0):
            off = plan_alr(capi, model, nrows, ncols, 1, it, LINE_SCAN)
        assert exact.family == off.family == "exact" and exact == off, what
        assert exact.nlaunch == sm.alr_exact_launches(model, nrows, ncols, it), what
        if lsc.scan_runs(model, nrows, ncols):
            assert scan.family == "scan" and scan.nlaunch == lsc.scan_launches(model, nrows, ncols, it), what
            assert (scan.cols.G, scan.rows.G) == (lsc.scan_groups(model, nrows), lsc.scan_groups(model, ncols)), what
        else:  # the documented fallback: exact order in both directions
            assert scan == exact, what


@pytest.mark.parametrize("model", sm.ALR_MODELS)
def test_what_every_plan_holds(capi, model):
    """Workspace, transposes, factor launches, field order and the sum of the launches, whatever the family."""
    nch, ntr, interior = sm.ALR[model]
    its = 1 if model == "pde8" else 3
    for (nrows, ncols), mode in itertools.product(SHAPES, (EXACT, RED_BLACK, LINE_SCAN)):
        with knobs():
            p = plan_alr(capi, model, nrows, ncols, 1, 3, mode)
        what = (model, nrows, ncols, mode)
        plane = nrows * ncols
        assert (p.ws_alr, p.ws_alr_t) == (8 * plane, (ntr + nch) * plane), what
        assert p.ws_aux1 == (plane if p.family == "zebra" else 0), what
        if p.family == "small":
            assert (p.nlaunch, p.coef_transposes, p.factor_launches, p.iterate_transposes) == (1, 0, 0, 0), what
            assert p.small_lds == sm.alr_small_lds_bytes(nrows, ncols, interior) and p.small_opt_in == (p.small_lds > 64 * KIB), what
            continue
        assert (p.coef_transposes, p.factor_launches, p.factor_pair, p.iterate_transposes) == (-(-ntr // sm.ALR_TB_MAX), 2, nch == 2, 2), what
        assert p.nlaunch == p.coef_transposes + p.factor_launches + its * (p.cols.launches + p.rows.launches + 2), what
        assert p.cols.order == (0, 1) and p.rows.order == ((1, 0) if nch == 2 else (0, 1)), what
        lo = 1 if interior else 0
        for q, n, nlines in ((p.cols, nrows, ncols), (p.rows, ncols, nrows)):
            assert (q.lo, q.hi, q.n, q.factor_grid) == (lo, nlines - 1 - lo, n, -(-(nlines - 2 * lo) // 8)), what
            assert q.opt_in == (q.lds > 64 * KIB) and q.launches * q.chains == nch * max(1, len(q.colours)), what


def test_no_shape_under_the_pixel_gate_reaches_the_lds_gate():
    """k_alr_small's 150 KiB gate never decides: the largest colour pass of a frame of up to 6144 pixels takes 20 bytes for about half
    its pixels (82 000 bytes at 3 x 2048), so the boundary has no shape to test."""
    worst = max(sm.alr_small_lds_bytes(r, c, False) for r in range(3, 2049) for c in range(3, sm.ALR_SMALL_MAX_PIXELS // r + 1))
    assert worst == sm.alr_small_lds_bytes(3, 2048, False) == 2 * 2049 * 20 < 150 * KIB


def test_the_pixel_gate(capi):
    """One single-field model here; the grid test holds all six to seam_model at the same shapes.  The gate's third clause, at most
    ALR_SMALL_MAXTR = 24 coefficient planes for k_alr_small's argument block, never decides either: the model with the most, llin8,
    has 15, so no call of the six entry points can fail it and no test here could."""
    assert max(ntr for _, ntr, _ in sm.ALR.values()) == 15 <= sm.ALR_SMALL_MAXTR
    with knobs():
        for shape, family in (((3, 2048), "small"), ((2048, 3), "small"), ((3, 2049), "zebra"), ((2049, 3), "zebra"), ((3, 3), "small")):
            assert plan_alr(capi, "disp4", *shape).family == family, shape
    with knobs(PDEIP_ALR_SMALL=0):
        assert plan_alr(capi, "disp4", 3, 3).family == "zebra"


def test_zebra_kernels_and_field_order(capi):
    with knobs(PDEIP_ALR_SMALL=0):
        pair, single = plan_alr(capi, "elin4", 3, 40), plan_alr(capi, "disp4", 3, 40)
    with knobs(PDEIP_ALR_SMALL=0, PDEIP_ALR_PAIR=0):
        per_field = plan_alr(capi, "elin4", 3, 40)
    for q in (pair.cols, pair.rows):
        assert (q.kernel, q.chains, q.launches, q.lds, q.opt_in) == ("k_alr_zebra3_pair", 2, 2, 2 * 7 * 8 * 100 * 4, False)
    for q in (per_field.cols, per_field.rows):
        assert (q.kernel, q.chains, q.launches) == ("k_alr_zebra3", 1, 4)
    assert (single.cols.kernel, single.cols.chains, single.cols.launches) == ("k_alr_zebra3", 1, 2)
    assert pair.nlaunch == 1 + 2 + 2 * (2 + 1 + 2 + 1) and per_field.nlaunch == 1 + 2 + 2 * (4 + 1 + 4 + 1)
    # 40 columns: lines 0, 2 .. 38 and 1, 3 .. 39, eight lines per workgroup; 3 rows: lines 0, 2 and line 1
    assert single.cols.colours == ((0, 38, 3), (1, 39, 3)) and single.cols.factor_grid == 5
    assert single.rows.colours == ((0, 2, 1), (1, 1, 1)) and single.rows.factor_grid == 1


def test_colours(capi):
    """The 9-point model relaxes interior lines only: one line, hence one colour, per direction at 3 x 3; a colour with no line
    makes no launch."""
    with knobs(PDEIP_ALR_SMALL=0):
        p3, p45 = plan_alr(capi, "pde8", 3, 3), plan_alr(capi, "pde8", 4, 5)
    assert p3.cols.colours == p3.rows.colours == ((1, 1, 1),) and p3.cols.launches == p3.rows.launches == 1
    assert p3.nlaunch == 1 + 2 + (1 + 1 + 1 + 1)
    assert p45.cols.colours == ((2, 2, 1), (1, 3, 1)) and p45.rows.colours == ((2, 2, 1), (1, 1, 1))
    assert p45.cols.launches == p45.rows.launches == 2 and p45.nlaunch == 1 + 2 + (2 + 1 + 2 + 1)


def test_exact_order_rules(capi):
    """Two chains of float4 share the 160 KiB up to lines of 5120 elements; one chain has them up to 10240; beyond, the line lives in
    global memory.  The rule is per direction."""
    with knobs():
        at, past = plan_alr(capi, "elin4", 5120, 3, mode=EXACT), plan_alr(capi, "elin4", 5121, 3, mode=EXACT)
        past2 = plan_alr(capi, "elin4", 5121, 3, mode=LINE_SCAN)
        g_at, g_past = plan_alr(capi, "pde4", 10240, 3, 2, mode=EXACT), plan_alr(capi, "pde4", 10241, 3, 2, mode=EXACT)
        first = plan_alr(capi, "elin4", 3, 3, mode=EXACT)
    assert (at.cols.kernel, at.cols.chains, at.cols.launches, at.cols.lds, at.cols.opt_in) == ("k_alr_lex", 2, 1, 160 * KIB, True)
    assert (past.cols.kernel, past.cols.chains, past.cols.launches, past.cols.lds, past.cols.opt_in) == ("k_alr_lex", 1, 2, 5121 * 16, True)
    assert (past.rows.kernel, past.rows.chains, past.rows.launches, past.rows.lds, past.rows.opt_in) == ("k_alr_lex", 2, 1, 2 * 3 * 16, False)
    assert past2 == past and past2.family == "exact"  # the scan's fallback: exact order in both directions
    assert (first.cols.chains, first.cols.launches, first.cols.lds) == (2, 1, 96) and first.nlaunch == 1 + 2 + 2 * 4
    assert (g_at.cols.kernel, g_at.cols.lds, g_at.cols.opt_in, g_at.ws_lex) == ("k_alr_lex", 160 * KIB, True, 0)
    assert (g_past.cols.kernel, g_past.cols.lds, g_past.cols.opt_in, g_past.cols.launches) == ("k_alr_lex global", 0, False, 1)
    assert g_past.ws_lex == 10241 * 4 * 2 and g_past.rows.kernel == "k_alr_lex" and g_past.cols.grid == g_past.rows.grid == 2
    with knobs():
        both = plan_alr(capi, "elin4", 10241, 3, mode=EXACT)
    assert (both.cols.kernel, both.cols.launches, both.rows.kernel, both.rows.launches) == ("k_alr_lex global", 2, "k_alr_lex", 1)


def test_scan_tree(capi):
    """G = ceil(line / (threads per chain * 4)): 2048 elements per group for two coupled fields, 4096 for one.  A coupled line of 6145
    would need a fourth group; the fallback (5120) takes it first."""
    G = lambda model, n: _scan(capi, model, n)
    assert [G("elin4", n) for n in (2048, 2049, 4096, 4097, 5120)] == [1, 2, 2, 3, 3]
    assert [G("disp4", n) for n in (4096, 4097, 5121, 8192, 8193, 10240)] == [1, 2, 2, 2, 3, 3]
    with knobs():
        for model, n in (("elin4", 5121), ("elin4", 6145), ("llin8", 6145), ("disp4", 10241), ("pde8", 10241)):
            assert plan_alr(capi, model, n, 3, mode=LINE_SCAN).family == "exact", (model, n)
            assert plan_alr(capi, model, 4, n, mode=LINE_SCAN).family == "exact", (model, n)


def _scan(capi, model, n):
    with knobs():
        p, t = plan_alr(capi, model, n, 3, mode=LINE_SCAN), plan_alr(capi, model, 5, n, mode=LINE_SCAN)
    nch = sm.ALR[model][0]
    for q in (p.cols, p.rows, t.cols, t.rows):
        assert (q.kernel, q.chains, q.launches, q.lds, q.opt_in, q.grid) == ("k_alr_scan", nch, 1, 0, False, 1)
    assert p.family == t.family == "scan" and p.rows.G == t.cols.G == 1 and p.cols.G == t.rows.G
    return p.cols.G


@pytest.mark.parametrize("model", sm.ALR_MODELS)
def test_knobs_are_read_only_on_their_path(capi, model):
    for nrows, ncols in ((3, 3), (64, 97), (5121, 3)):
        plans = {}
        for env in ({}, dict(PDEIP_ALR_SCAN=0), dict(PDEIP_ALR_SMALL=0), dict(PDEIP_ALR_PAIR=0)):
            with knobs(**env):
                plans[tuple(env)] = [plan_alr(capi, model, nrows, ncols, mode=m) for m in (EXACT, RED_BLACK, LINE_SCAN)]
        base = plans[()]
        assert plans[("PDEIP_ALR_SCAN",)][EXACT] == base[EXACT] and plans[("PDEIP_ALR_SCAN",)][RED_BLACK] == base[RED_BLACK]
        assert plans[("PDEIP_ALR_SMALL",)][EXACT] == base[EXACT] and plans[("PDEIP_ALR_SMALL",)][LINE_SCAN] == base[LINE_SCAN]
        assert plans[("PDEIP_ALR_PAIR",)][EXACT] == base[EXACT] and plans[("PDEIP_ALR_PAIR",)][LINE_SCAN] == base[LINE_SCAN]
        if sm.ALR[model][0] == 1:
            assert plans[("PDEIP_ALR_PAIR",)] == base


@pytest.mark.parametrize("mode", (EXACT, RED_BLACK, LINE_SCAN))
def test_nothing_to_do_and_the_nine_point_models_one_iteration(capi, mode):
    with knobs():
        for model in sm.ALR_MODELS[:-1]:
            for it in (0, -1):
                p = plan_alr(capi, model, 9, 11, 1, it, mode)
                assert (p.family, p.nlaunch, p.ws_alr, p.cols.kernel) == (None, 0, 0, None), (model, it)
        one = plan_alr(capi, "pde8", 64, 97, 2, 1, mode)
        assert one.family is not None and one.nlaunch > 0
        for it in (7, 0):  # its entry point runs one iteration whatever `iter` says
            assert plan_alr(capi, "pde8", 64, 97, 2, it, mode) == one
