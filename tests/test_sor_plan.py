"""CPU: the library's own launch plan of a point-SOR call (pdeip_debug_plan_sor, csrc/pdeip_sor_plan.hpp) against the independent
model of tests/seam_model.py -- family, launch count, sweeps per launch, strip / tile geometry, buffers, strip-width pickers and
the exact-order forms.  The device facts are passed (256 compute units, explicit slot counts), so no GPU is asked."""
import itertools
import random

import pytest

import seam_model as sm
from sor_plan import CALLER, DST, SCRATCH, knobs, plan_sor, point_case_knobs

EXACT, RED_BLACK, LINE_SCAN = 0, 1, 2


@pytest.fixture(scope="module")
def capi(pdeip):
    return pdeip.capi


def _ceil(a, b):
    return (a + b - 1) // b


def check_geometry(model, nrows, ncols, aligned, launch):
    g = sm.geometry(launch.kernel, model, nrows, ncols, launch.tj, aligned=aligned)
    assert (launch.tiles, launch.units, launch.grid) == (g.row_tiles, g.row_tiles * g.strips, g.grid), (launch, g)


@pytest.mark.parametrize("c", sm.CASES, ids=sm.case_id)
def test_every_seam_case(capi, c):
    """Under the knobs run_point_case sets: the family, the launch count, the sweeps per launch, and tiles / strips / grid of every
    launch as geometry() gives them for the kernel that launch runs, at the forced width where the case forces one."""
    with knobs(**point_case_knobs(c)):
        p = plan_sor(capi, c.model, c.nrows, c.ncols, c.nframes, c.it, aligned=c.role is None, has_dst=not c.inplace)
    family = sm.expected_family(c)
    assert family == c.family and p.family == family
    assert len(p.launches) == sm.expected_launches(c)
    runs = 2 if c.model == "dispsym4" else 1  # the entry point runs its plan twice
    sweeps = [l.sweeps for l in p.launches]
    if family == "small":
        per = c.it if len(sweeps) == runs else 4
        assert sweeps == runs * ([per] * (c.it // per) + ([c.it % per] if c.it % per else []))
        assert {l.kernel for l in p.launches} == {"k_sor_small"}
        return
    assert sweeps == runs * sm.chain(family, c.it)
    nine = c.model == "pde8"
    by_sweeps = {4: "k_sor_rbp", 2: "k_pde8_colour2" if nine else "k_sor_rb two-sweep", 1: "k_pde8_colour" if nine else "k_sor_rb one-sweep"}
    assert [l.kernel for l in p.launches] == [by_sweeps[k] for k in sweeps]
    assert set(sm.kernels_of(family, c.it)) <= {l.kernel for l in p.launches}
    forced = sm.case_geometries(c)
    for l in p.launches:
        check_geometry(c.model, c.nrows, c.ncols, c.role is None, l)
        if l.kernel in forced:
            assert l.tj == c.tj, l


GRID_ROWS = (3, 4, 5, 8, 236, 240, 241, 244, 248, 249, 342, 343, 484)
GRID_COLS = (3, 8, 9, 26, 79, 342, 2047, 2048, 8744)


@pytest.mark.parametrize("model", list(sm.MODELS))
def test_family_and_launch_count_over_a_grid_of_shapes(capi, model):
    for small, pipe in itertools.product((True, False), repeat=2):
        with knobs(PDEIP_RB_SMALL=int(small), PDEIP_RB_PIPE=int(pipe)):
            for nrows, ncols, it, aligned in itertools.product(GRID_ROWS, GRID_COLS, sm.ITERS, (True, False)):
                p = plan_sor(capi, model, nrows, ncols, 1, it, aligned=aligned)
                family = sm.family_of(model, nrows, ncols, 1, it, small=small, pipe=pipe, aligned=aligned)
                what = (model, nrows, ncols, it, small, pipe, aligned)
                assert p.family == family, what
                assert len(p.launches) == sm.sweep_launches(family, model, nrows, ncols, 1, it), what


@pytest.mark.parametrize("model", list(sm.MODELS))
def test_single_field_models_enter_the_pipeline_at_two_to_the_21_pixels(capi, model):
    with knobs(PDEIP_RB_SMALL=0):
        below, at = (plan_sor(capi, model, 1024, ncols, 1, 8).family for ncols in (2047, 2048))
    assert 1024 * 2048 == sm.PIPE_MIN_PIXELS
    want = {"coupled": ("rbp", "rbp"), "single": ("rb", "rbp"), "pde8": ("pde8", "pde8")}[sm.CLASS[model]]
    assert (below, at) == want


@pytest.mark.parametrize("model,env", [("elin4", dict(PDEIP_RB_PIPE=0)), ("elin4", {}), ("disp4", {}), ("pde8", {})])
def test_buffer_rule(capi, model, env):
    """rb, rbp (from four sweeps on) and the four-colour chain: the launches ping-pong."""
    for it, has_dst in itertools.product(range(1, 10), (False, True)):
        if model == "pde8" and has_dst:
            continue  # the entry point has no destination
        with knobs(PDEIP_RB_SMALL=0, **env):
            p = plan_sor(capi, model, 8, 40, 1, it, has_dst=has_dst)
        assert p.family in ("rb", "rbp", "pde8") and not p.opening_copy
        ls = p.launches
        assert ls[0].src == CALLER and all(b.src == a.dst for a, b in zip(ls, ls[1:]))
        if has_dst:
            assert all(l.src != CALLER for l in ls[1:]) and all(l.dst != CALLER for l in ls)
            assert ls[-1].dst == DST and not p.closing_copy
        else:
            assert all(l.dst in (CALLER, SCRATCH) and l.src != DST for l in ls)
            assert p.closing_copy == (len(ls) % 2 == 1) == (ls[-1].dst == SCRATCH)


def test_picker_at_4k(capi):
    """2160 x 3840 elin4 on 256 resident workgroups."""
    with knobs(PDEIP_RB_SMALL=0):
        first = plan_sor(capi, "elin4", 2160, 3840, 1, 4, rbp_slots=256).launches[0]
    assert (first.kernel, first.tj, first.units) == ("k_sor_rbp", 138, 252)  # 157 steps = TJ + 5 * 4 - 1: the record carries no step count


def test_pickers_choose_the_cheapest_width(capi):
    """k_sor_rbp: the smallest TJ in 8..1024 that reaches the minimum of ceil(units / slots) * nsteps(TJ); the two-sweep march: the
    largest in 2..64 that reaches the minimum of ceil(units / slots) * (TJ + 6)."""
    rng = random.Random(4242)
    for _ in range(20):
        nrows, ncols, nframes = 4 * rng.randint(1, 600), rng.randint(3, 5000), rng.choice((1, 1, 3))
        slots_p, slots_2 = rng.randint(1, 1024), rng.randint(1, 16384)
        with knobs(PDEIP_RB_SMALL=0):
            p = plan_sor(capi, "pde4" if nframes > 1 else "llin4", nrows, ncols, nframes, 6, rb2_slots=slots_2, rbp_slots=slots_p)
        if p.family == "rb":  # pde4 below 2^21 pixels
            assert nframes > 1 and nrows * ncols < sm.PIPE_MIN_PIXELS
        else:
            tiles = _ceil(nrows, sm.RBP_OWN_ROWS)
            cost = {tj: _ceil(tiles * _ceil(ncols, tj) * nframes, slots_p) * (tj + 5 * sm.RBP_S - 1) for tj in range(8, 1025)}
            assert p.launches[0].kernel == "k_sor_rbp" and p.launches[0].tj == min(tj for tj in cost if cost[tj] == min(cost.values()))
        tiles = _ceil(nrows - 1, sm.RB_OWN_ROWS)
        cost = {tj: _ceil(tiles * _ceil(ncols, tj) * nframes, slots_2) * (tj + 6) for tj in range(2, 65)}
        assert p.launches[-1].kernel == "k_sor_rb two-sweep" and p.launches[-1].tj == max(tj for tj in cost if cost[tj] == min(cost.values()))


def test_a_forced_width_below_two_becomes_two(capi):
    with knobs(PDEIP_RB_SMALL=0, PDEIP_RBP_TJ=1, PDEIP_RB_TJ=1):
        p = plan_sor(capi, "elin4", 8, 40, 1, 7)
        p8 = plan_sor(capi, "pde8", 8, 40, 1, 3)
    assert [l.sweeps for l in p.launches] == [4, 2, 1] and [l.sweeps for l in p8.launches] == [2, 1]
    assert {l.tj for l in p.launches + p8.launches} == {2}


@pytest.mark.parametrize("model", ["elin4", "disp4", "dispsym4", "pde8"])
def test_exact_order_form(capi, model):
    """Persistent by default, per front under PDEIP_EXACT_PERSIST=0 / PDEIP_PDE8_PERSIST=0 and where a 16-bit field would not fit,
    the walker only under PDEIP_EXACT_WALK=1; LINE_SCAN plans as exact order.  Launch counts as seam_model.exact_launches."""
    form = lambda ncols=70, mode=EXACT, **env: _exact(capi, model, ncols, mode, env)
    assert form() == form(mode=LINE_SCAN) == "persist"
    assert form(PDEIP_EXACT_PERSIST=0, PDEIP_PDE8_PERSIST=0) == "front"
    assert form(PDEIP_EXACT_WALK=1) == ("persist" if model == "pde8" else "walk")
    assert form(PDEIP_EXACT_WALK=1, PDEIP_EXACT_PERSIST=0) == ("persist" if model == "pde8" else "front")
    assert form(ncols=65535) == "persist" and form(ncols=65536) == "front"


def _exact(capi, model, ncols, mode, env):
    with knobs(**env):
        p = plan_sor(capi, model, 37, ncols, 1, 4, mode=mode, has_dst=model != "pde8")
    assert p.family == "exact" and not p.closing_copy and p.opening_copy == (model != "pde8")
    assert p.persist_setup == (p.form != "front")
    assert len(p.launches) == sm.exact_launches(model, 37, ncols, 4, p.form)
    return p.form
