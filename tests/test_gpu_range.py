"""GPU: every site that derives a reciprocal, on problems whose divisors leave the range of ordinary numbers -- bit for bit against
the oracle.

tests/problems.py gives every kernel divisors between about 2 and 25.  tests/range_problems.py laces the same problems with
divisor data of +-3e38 and +Inf (reciprocal subnormal or zero), weights of exactly 0.0f and -0.0f, subnormal and negative-zero
right-hand sides and iterates, NaN on pixels of its own and, for point SOR, one pixel whose denominator is subnormal (its
reciprocal overflows).  tests/test_range_problems.py shows on the CPU that the oracle equals the reference's own gateways on these
problems, that every output plane of every case here stays >= 99 % finite, that the outputs hold subnormals and -0.0, and that
the pipeline cases mix clean and fallback waves.  Half the cases run omega = 1, where the stored value is 0 c + 1 (a div) and
the reciprocal's bits go straight to the output.

The families are forced by the knobs of tests/test_gpu_seams.py (set through its knobs() context and restored), the cases are
seam_model's RANGE_* lists, and the launch counts are the model's: a case that falls to another family fails on its count.
k_sor_rbp is the one kernel with two reciprocals -- v_rcp_f32 + one Newton step, and the IEEE division for a wave that ballots a
lane outside [2^-126, 2^126): RANGE_RBP runs launches in which some waves take each branch, launches in which none falls back
and launches in which all do.  Line relaxation gets no subnormal denominator (class T): a Thomas solve carries the Inf along
whole lines, and every output of the call would be non-finite.
"""
import functools

import numpy as np
import pytest

import problems as pb
import seam_model as sm
from test_gpu_seams import knobs, run_point_case
from test_range_problems import GATEWAY, gateway_problem, gateway_want, problem_of

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(autouse=True)
def exact_mode_afterwards(pdeip):
    yield
    pdeip.mex_api.set_mode(pdeip.MODE_EXACT_ORDER)


@functools.lru_cache(maxsize=None)
def want_through_gateway(model, nrows, ncols, nframes, corner, it, omega, solver, order):
    """Computed once, shared by the forms of a kernel that must all give it, and never written."""
    return gateway_want(model, gateway_problem(model, nrows, ncols, nframes, corner), it, omega, solver, order)


def check_gateway(pdeip, model, p, want, it, omega, solver, what):
    api = pdeip.mex_api
    kw = {} if model in ("pde4", "pde8") else {"nargout": len(want)}
    got = getattr(api, GATEWAY[model])(*p.values(), F32(it), F32(omega), F32(solver), **kw)
    launches = pdeip.capi.load().pdeip_last_launch_count()
    got = got if isinstance(got, tuple) else (got,)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert pb.bit_equal(g, w), "%s output %d: %s" % (what, k, pb.describe_mismatch(g, w))
    return launches


# ---- point SOR, red-black order ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rc", sm.RANGE_SMALL, ids=sm.range_case_id)
def test_small_path(pdeip, oracle, rc):
    """k_sor_small with the knobs at their defaults: the whole call in one launch, or four sweeps per launch on a cut frame."""
    run_point_case(pdeip, oracle, rc.case, problem=problem_of(rc), omega=rc.omega)


@pytest.mark.parametrize("rc", sm.RANGE_RB, ids=sm.range_case_id)
def test_marches_and_four_colour_kernels(pdeip, oracle, rc):
    """k_sor_rb and k_pde8_colour / k_pde8_colour2 (PDEIP_RB_SMALL=0, PDEIP_RB_PIPE=0, PDEIP_RB_TJ in {3, 13}): iter 1, 2, 3 run the
    one-sweep kernel alone, the two-sweep kernel alone -- whose first launch derives -- and both."""
    run_point_case(pdeip, oracle, rc.case, problem=problem_of(rc), omega=rc.omega)


@pytest.mark.parametrize("rc", sm.RANGE_RBP, ids=sm.range_case_id)
def test_pipeline_ballot(pdeip, oracle, rc):
    """k_sor_rbp: waves that keep the fast reciprocal beside waves that redo their lanes with the division (div_frac 0.002), none
    that falls back (0), none that stays clean (0.1); one-field waves of the coupled models (WHICH = 1 / 2), the single-field models
    at the 2^21 switch, disp4 mirrored, whose derive() adds wE before wW."""
    run_point_case(pdeip, oracle, rc.case, problem=problem_of(rc), omega=rc.omega)


# ---- point SOR, exact order, through the gateways -------------------------------------------------------------------------------

EXACT_RUNS = [(f, e) for m in sm.RANGE_EXACT_MODELS for f in sm.exact_forms(m) for e in sm.range_exact_cases(m)]


@pytest.mark.parametrize("form,e", EXACT_RUNS, ids=lambda v: v if isinstance(v, str) else "-".join(str(x) for x in v))
def test_exact_order_forms(pdeip, form, e):
    """k_pack_coefficients + k_sor_exact_persist (the default), k_derive + k_sor_exact (PDEIP_EXACT_PERSIST=0), the walkers' loader
    (PDEIP_EXACT_WALK=1), pde8 on both settings of PDEIP_PDE8_PERSIST: every output the gateway has, residuals included.  The launch
    count tells the launch-per-front form from the persistent ones; the walker and k_sor_exact_persist both make three launches, and
    only the knob, which the library reads in every call, sets them apart."""
    pdeip.mex_api.set_mode(pdeip.MODE_EXACT_ORDER)
    p = gateway_problem(e.model, e.nrows, e.ncols, e.nframes, e.corner)
    want = want_through_gateway(e.model, e.nrows, e.ncols, e.nframes, e.corner, e.it, e.omega, 1, 0)
    with knobs(**sm.EXACT_FORMS[form]):
        launches = check_gateway(pdeip, e.model, p, want, e.it, e.omega, 1, "%s %s" % (form, tuple(e)))
    expect = sm.exact_launches(e.model, e.nrows, e.ncols, e.it, form)
    assert launches == expect, "%s %s: %d launches, the %s form makes %d" % (form, tuple(e), launches, form, expect)
    assert pdeip.capi.load().pdeip_persist_error() == 0


# ---- line relaxation ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("a", [a for m in sm.ALR_MODELS for a in sm.range_alr_cases(m)], ids=lambda a: "-".join(str(x) for x in a))
def test_line_relaxation(pdeip, a):
    """The Thomas recurrences of pdeip_alr.hpp.  Exact order: both chains of a coupled model in one launch, and one chain per launch
    on lines of 5200 elements.  Zebra: k_alr_small, then k_alr_zebra3 / k_alr_zebra3_pair (PDEIP_ALR_SMALL=0, coupled models also with
    PDEIP_ALR_PAIR=0).  Launch counts as run_alr makes them."""
    pdeip.mex_api.set_mode(pdeip.MODE_RED_BLACK if a.zebra else pdeip.MODE_EXACT_ORDER)
    p = gateway_problem(a.model, a.nrows, a.ncols, a.nframes)
    want = want_through_gateway(a.model, a.nrows, a.ncols, a.nframes, False, a.it, a.omega, 2, 1 if a.zebra else 0)
    with knobs(PDEIP_ALR_SMALL=None if a.small else 0, PDEIP_ALR_PAIR=None if a.pair else 0):
        launches = check_gateway(pdeip, a.model, p, want, a.it, a.omega, 2, "alr %s" % (tuple(a),))
    if a.zebra:
        expect = sm.alr_launches(a.model, a.nrows, a.ncols, a.it, small=a.small, pair=a.pair)
        assert (expect == 1) == (a.small and sm.alr_family(a.model, a.nrows, a.ncols, True) == "alr_small")
    else:
        expect = sm.alr_exact_launches(a.model, a.nrows, a.ncols, a.it)
    assert launches == expect, "%s: %d launches, run_alr makes %d" % (tuple(a), launches, expect)
