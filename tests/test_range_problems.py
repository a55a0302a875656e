"""CPU: the range-laced problems (tests/range_problems.py) are a fair yardstick.

Four things are shown here, without a GPU, about the problems that tests/test_gpu_range.py sends through every derive site:

  * the oracle still equals the reference's own compiled gateways on them, bit for bit, in the reference's order, for both
    solvers and every nlhs -- so "bit for bit against the oracle" means the same at these values as at ordinary ones;
  * in every case the GPU module runs, every output plane the oracle gives, in the order that case compares, is at least 99 %
    finite: any NaN equals any NaN in bit_equal, and a test must not hide behind that;
  * the outputs really hold what the lacing is for: subnormal values, and the negative zeros bit_equal tells from +0.0;
  * a launch of k_sor_rbp on the mixed pipeline cases has waves that keep v_rcp_f32 + Newton beside waves that take the IEEE
    division; on the clean cases none falls back, on the all-fallback cases none stays clean.

`-s` shows the measured figures.
"""
import functools

import numpy as np
import pytest

import oracle_lib as orc
import problems as pb
import range_problems as rp
import ref_lib
import seam_model as sm
from test_gpu_seams import want_of
from test_ref_oracle import NLHS, _build_ref_module, same

F32 = np.float32
GATEWAY = {"elin4": "Oflow_sor_elin4_2d", "llin4": "Oflow_sor_llin4_2d", "llin8": "Oflow_sor_llin8_2d", "disp4": "Disp_sor_llin4_2d",
           "dispsym4": "Disp_sor_llin_sym4_2d", "pde4": "PDEsolver4", "pde8": "PDEsolver8"}
FINITE_CAP = 0.99
MIN_SUBNORMAL_MODELS = tuple(GATEWAY)
MIN_NEGZERO_MODELS = ("elin4", "llin4", "llin8", "disp4", "dispsym4")  # the reference gives pde4 and pde8 no -0.0 at these inputs


# ---- what both range modules share ---------------------------------------------------------------------------------------------

def nan_frac_of(nrows, ncols):
    return 0.02 if nrows * ncols < sm.PIPE_MIN_PIXELS else 0.005


@functools.lru_cache(maxsize=4)
def laced(model, nrows, ncols, nframes=1, frac=0.01, div_frac=None, corner=False):
    """The problem of a case; shared and never written (every consumer copies: oracle_lib.F, device.to_device)."""
    return rp.range_laced(model, sm.RANGE_SEED, nrows, ncols, nframes, frac=frac, div_frac=div_frac, nan_frac=nan_frac_of(nrows, ncols), corner=corner)


def lacing_census(model, p):
    return rp.census(model, p)


def problem_of(rc):
    """rc: a seam_model.RangeCase."""
    c = rc.case
    return laced(c.model, c.nrows, c.ncols, c.nframes, rc.frac, rc.div_frac, rc.corner)


def gateway_problem(model, nrows, ncols, nframes=1, corner=False):
    """The problem of a case that goes through a gateway with its residual outputs: see seam_model.RANGE_GATEWAY_DIV."""
    return laced(model, nrows, ncols, nframes, 0.01, sm.RANGE_GATEWAY_DIV, corner)


def gateway_want(model, p, it, omega, solver, order, nlhs=None):
    """The oracle's gateway-level result, as a tuple, with the most outputs the gateway has (the residuals see the specials too)."""
    gw = GATEWAY[model]
    kw = {} if gw.startswith("PDE") else {"nargout": max(NLHS[gw]) if nlhs is None else nlhs}
    out = getattr(orc, gw)(*p.values(), it, omega, solver=solver, order=order, **kw)
    return out if isinstance(out, tuple) else (out,)


# ---- reference agreement ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ref_build():
    """The rule of test_ref_oracle.py: with a reference checkout at hand a missing or stale oracle/_ref/ is a failure; only when
    neither the checkout nor a build exists do the comparisons with the reference skip."""
    br = _build_ref_module()
    tree = br.reference_dir()
    if tree is not None:
        if not br.up_to_date(tree):
            pytest.fail("oracle/_ref/ is missing or stale against the reference at %s: run `python __graft_entry__.py build`" % tree)
    elif ref_lib.available() is None:
        pytest.skip("no reference checkout and no oracle/_ref/ build: nothing to compare the oracle with")
    assert ref_lib.available() is not None


REF_SHAPES = [(5, 300), (260, 7), (131, 70), (244, 300)]
REF_ITERS = (1, 4, 9)
REF_FRAC = {(5, 300): 0.02, (260, 7): 0.02}  # tiny frames: a larger share, so that every class occupies a pixel


@pytest.mark.parametrize("shape", REF_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("solver", [1, 2])
@pytest.mark.parametrize("model", list(GATEWAY))
def test_oracle_matches_the_reference_on_range_laced_problems(ref_build, model, solver, shape):
    gw = GATEWAY[model]
    frames = 2 if model in ("pde4", "pde8") and shape == (131, 70) else 1
    corner = solver == 1 and shape[0] * shape[1] >= rp.CORNER_MIN_PIXELS  # class T: the reference's point SOR meets it too
    p = laced(model, shape[0], shape[1], frames, REF_FRAC.get(shape, 0.01), None, corner)
    census = lacing_census(model, p)
    assert all(n > 0 for n in census.values()) and ("T" in census) == corner
    for it in REF_ITERS:
        for omega in (1.0, 1.9 if solver == 1 else 1.4):
            for nlhs in NLHS[gw]:
                got = ref_lib.call(gw, nlhs, *p.values(), F32(it), F32(omega), F32(solver))
                same(got, gateway_want(model, p, it, omega, solver, orc.LEX, nlhs), "%s %s solver %d iter %d omega %g nlhs %d" % (gw, shape, solver, it, omega, nlhs))


# ---- every case of tests/test_gpu_range.py, on the CPU ---------------------------------------------------------------------------

def gpu_runs():
    """(id, model, omega, lacing (frac, div_frac, corner), thunk -> (problem, the oracle's outputs in the order the case compares))
    for every comparison the GPU module makes; cases that differ only in what forces the kernel family share one entry."""
    runs = {}

    def add(key, model, omega, lacing, thunk):
        runs.setdefault(key, (model, omega, lacing, thunk))

    for rc in sm.RANGE_CASES:
        c = rc.case
        add(("sor-colour", c.model, c.nrows, c.ncols, c.nframes, c.it, rc.omega, c.col0, rc.frac, rc.div_frac), c.model, rc.omega,
            (rc.frac, rc.div_frac, rc.corner), lambda rc=rc: (problem_of(rc), want_of(orc, rc.case.model, problem_of(rc), rc.case.it, rc.case.col0, rc.omega)))
    for model in sm.RANGE_EXACT_MODELS:
        for e in sm.range_exact_cases(model):
            add(("sor-lex",) + tuple(e), model, e.omega, (0.01, sm.RANGE_GATEWAY_DIV, e.corner),
                lambda e=e: (gateway_problem(e.model, e.nrows, e.ncols, e.nframes, e.corner),
                             gateway_want(e.model, gateway_problem(e.model, e.nrows, e.ncols, e.nframes, e.corner), e.it, e.omega, 1, orc.LEX)))
    for model in sm.ALR_MODELS:
        for a in sm.range_alr_cases(model):
            add(("alr", a.model, a.nrows, a.ncols, a.nframes, a.it, a.omega, a.zebra), model, a.omega, (0.01, sm.RANGE_GATEWAY_DIV, False),
                lambda a=a: (gateway_problem(a.model, a.nrows, a.ncols, a.nframes),
                             gateway_want(a.model, gateway_problem(a.model, a.nrows, a.ncols, a.nframes), a.it, a.omega, 2, orc.COLOUR if a.zebra else orc.LEX)))
    return runs


@pytest.fixture(scope="module")
def survey():
    """Every run once: per run the finite share of each output plane, the subnormal and negative-zero counts, the lacing's census."""
    out = []
    for key, (model, omega, lacing, thunk) in gpu_runs().items():
        p, want = thunk()
        shares = [float(np.isfinite(w).mean()) for w in want]
        flat = np.concatenate([np.ravel(w) for w in want])
        tiny = int(((flat != 0) & (np.abs(flat) < np.finfo(F32).tiny)).sum())
        negzero = int(((flat == 0) & np.signbit(flat)).sum())
        out.append(dict(key=key, model=model, omega=omega, lacing=lacing, shares=shares, subnormal=tiny, negzero=negzero,
                        census=lacing_census(model, p)))
    return out


def test_every_gpu_case_stays_finite(survey):
    """The cap against a test that hides behind NaN: >= 99 % of every output plane is finite, in the order the case compares."""
    worst = min(survey, key=lambda r: min(r["shares"]))
    by_kind = {}
    for r in survey:
        by_kind[r["key"][0]] = min(by_kind.get(r["key"][0], 1.0), min(r["shares"]))
    print("\nfinite share: %d runs, lowest per kind %s; lowest of all %.5f at %s" % (len(survey), {k: round(v, 5) for k, v in by_kind.items()}, min(worst["shares"]), worst["key"]))
    bad = [(r["key"], r["shares"]) for r in survey if min(r["shares"]) < FINITE_CAP]
    assert not bad, "output planes less than %g finite: %s" % (FINITE_CAP, bad[:5])


def test_outputs_hold_subnormals_and_negative_zeros(survey):
    """For each model at least one omega = 1 case whose result holds a subnormal value, and (but for pde4 / pde8) one that holds -0.0:
    at omega = 1 the stored value is 0 c + 1 (a div), so a flushed subnormal or a lost sign of zero reaches the output."""
    for model in MIN_SUBNORMAL_MODELS:
        mine = [r for r in survey if r["model"] == model and r["omega"] == 1.0]
        sub, neg = [r["subnormal"] for r in mine], [r["negzero"] for r in mine]
        print("\n%s: %d omega = 1 runs; subnormal outputs per run min %d max %d, -0.0 outputs per run min %d max %d" % (model, len(mine), min(sub), max(sub), min(neg), max(neg)))
        assert max(sub) > 0, model
        if model in MIN_NEGZERO_MODELS:
            assert max(neg) > 0, model


def test_every_class_occupies_a_pixel_in_every_case(survey):
    """...but the three out-of-range divisor classes of a case that is meant to have none (div_frac = 0)."""
    for r in survey:
        frac, div_frac, corner = r["lacing"]
        for cls, n in r["census"].items():
            if div_frac == 0 and cls in rp.DIV_CLASSES:
                assert n == 0, (r["key"], cls)
            else:
                assert n > 0, (r["key"], cls)
        assert ("T" in r["census"]) == corner
    assert any(r["lacing"][2] for r in survey) and not any(r["lacing"][2] for r in survey if r["key"][0] == "alr")  # class T: point SOR only


@pytest.mark.parametrize("order", ["lex", "colour"])
@pytest.mark.parametrize("model", ["elin4", "llin4", "disp4", "dispsym4", "pde4", "pde8"])
def test_class_t_reaches_the_outputs(model, order):
    """The subnormal denominator sits on a pixel point SOR relaxes: the oracle's result with class T differs from the result
    without it and holds an Inf or NaN near that pixel, and nothing changes further away than a non-finite value can travel: one
    pixel per sweep in lexicographic order, one per half-sweep in colour order (seam_model.corner_fits counts on that)."""
    it, nrows, ncols = 4, 131, 70
    a, b = laced(model, nrows, ncols, 1, 0.01, None, True), laced(model, nrows, ncols, 1, 0.01, None, False)
    if order == "lex":
        wa, wb = gateway_want(model, a, it, 1.0, 1, orc.LEX, NLHS[GATEWAY[model]][0]), gateway_want(model, b, it, 1.0, 1, orc.LEX, NLHS[GATEWAY[model]][0])
    else:
        wa, wb = want_of(orc, model, a, it, 0, 1.0), want_of(orc, model, b, it, 0, 1.0)
    # (the 9-point stencil hands it on twice within a lexicographic sweep: a pixel reads its north-east neighbour's new value)
    reach = (4 if model == "pde8" else 2) * it if order == "colour" else (2 if model == "pde8" else 1) * it
    near = np.zeros((nrows, ncols), bool)
    near[nrows - 2 - reach:, ncols - 2 - reach:] = True
    hit = 0
    for ga, gb in zip(wa, wb):
        same_bits = (ga.view(np.uint32) == gb.view(np.uint32)) | (np.isnan(ga) & np.isnan(gb))
        assert same_bits[~near].all(), "%s %s: class T changed a pixel more than %d away" % (model, order, reach)
        hit += int((~np.isfinite(ga[near]) & np.isfinite(gb[near])).sum())
    assert hit > 0, "%s %s: class T made no output non-finite" % (model, order)


def test_classes_are_disjoint_and_hold_their_values():
    p = rp.range_laced("elin4", 7, 131, 70, 2, corner=True)
    masks = rp.class_map(7, 131, 70)
    assert int(sum(m.astype(int) for m in masks.values()).max()) == 1
    m = masks["H-"]
    assert (p["Du"][m] == F32(-3e38)).all() and (p["Dv"][m] == F32(-3e38)).all() and np.isfinite(p["Cu"][m]).all()
    for k in rp.W4:
        assert np.signbit(p[k][masks["Z-"]]).all() and (p[k][masks["Z-"]] == 0).all() and not np.signbit(p[k][masks["Z"]]).any()
    assert (p["wE"][masks["E0"]] == 0).all() and (p["wW"][masks["E0"]] != 0).all() and np.signbit(p["wW"][masks["W-"]]).all()
    assert (p["Cu"][masks["C"]] == F32(1e-41)).all() and (p["M"][masks["C"]] == F32(1e-41)).all() and F32(1e-41) > 0
    assert (p["U"][masks["X"]] == F32(3e-42)).all() and np.signbit(p["V"][masks["X-"]]).all()
    expect = masks["N"].copy()
    expect[rp.CORNER] = False  # class T takes its pixel from whatever class held it
    assert np.array_equal(np.isnan(p["Du"][..., 1]), expect) and np.array_equal(np.isnan(p["M"][..., 0]), expect) and not np.isnan(p["wW"]).any()
    assert p["Du"][-2, -2, 0] == F32(1e-39) and p["wN"][-2, -2] == 0
    d = rp.divisors("elin4", p)
    assert d.shape == (2, 131, 70) and not rp.in_fast_range(d[:, -2, -2]).any()  # class T: a subnormal denominator
    assert not rp.in_fast_range(d[0][masks["H+"] | masks["H-"] | masks["I"]]).any()
    clean = ~(masks["H+"] | masks["H-"] | masks["I"])
    clean[rp.CORNER] = False
    assert rp.in_fast_range(d[:, clean]).all()
    assert list(rp.in_fast_range(np.array([0.0, -0.0, np.nan, np.inf, 1e-39, 2.0 ** -126, -(2.0 ** 125), 2.0 ** 126], F32))) == [False] * 5 + [True, True, False]


@pytest.mark.parametrize("model", rp.MODELS)
def test_divisors_restate_derive(model):
    """On an ordinary problem the divisor is the sum of derive(), in its association order, and inside the fast range."""
    p = rp.range_laced(model, 3, 24, 20, nan_frac=0.0, frac=0.0)
    d = rp.divisors(model, p)
    if model in ("pde4", "pde8"):
        assert pb.bit_equal(d[0], p["TRACE"])
    elif model == "disp4":
        assert pb.bit_equal(d[0], (((p["Du"] + p["wE"]) + p["wW"]) + p["wS"]) + p["wN"])
    elif model == "dispsym4":
        assert d.shape[0] == 2 and pb.bit_equal(d[1], (((p["Du1"] + p["wE1"]) + p["wW1"]) + p["wS1"]) + p["wN1"])
    else:
        assert d.shape[0] == 2 and pb.bit_equal(d[1], ((p["wW"] + p["wE"]) + (p["wN"] + p["wS"])) + p["Dv"])
    assert rp.in_fast_range(d).all()


def test_pipeline_cases_mix_clean_and_fallback_waves():
    """(column, 240-row tile) groups that hold an out-of-range divisor, as a share of all: within [0.2, 0.95] for the mixed cases, so
    both branches of the ballot run in one launch; 0 for the clean, 1 for the all-fallback cases.  Approximate geometry (the 16
    halo lanes of a wave are ignored)."""
    seen = set()
    for rc in sm.RANGE_RBP:
        c = rc.case
        assert c.family == "rbp" and c.nrows >= sm.RBP_OWN_ROWS
        share = rp.fallback_group_share(c.model, problem_of(rc), sm.RBP_OWN_ROWS)
        print("\n%s: %.3f of the groups fall back" % (sm.range_case_id(rc), share))
        if rc.div_frac == sm.RANGE_CLEAN:
            assert share == 0.0, sm.range_case_id(rc)
        elif rc.div_frac == sm.RANGE_FALLBACK:
            assert share == 1.0, sm.range_case_id(rc)
        else:
            assert 0.2 <= share <= 0.95, (sm.range_case_id(rc), share)
        seen.add((c.model, rc.div_frac))
    assert seen == {(m, d) for m in ("elin4", "llin4", "disp4", "pde4", "dispsym4") for d in (sm.RANGE_MIXED, sm.RANGE_CLEAN, sm.RANGE_FALLBACK)}


def test_range_cases_reach_what_the_families_need():
    """The lists of seam_model against what they are for: the family the model predicts, omega = 1 in every family for every model, and
    the knob values each family is to meet."""
    for rc in sm.RANGE_CASES:
        assert sm.expected_family(rc.case) == rc.case.family, sm.range_case_id(rc)
    assert len({sm.range_case_id(rc) for rc in sm.RANGE_CASES}) == len(sm.RANGE_CASES)
    for cases, models in ((sm.RANGE_SMALL, ("elin4", "llin4", "disp4", "dispsym4", "pde4")), (sm.RANGE_RB, ("elin4", "llin4", "disp4", "dispsym4", "pde4", "pde8")),
                          (sm.RANGE_RBP, ("elin4", "llin4", "disp4", "dispsym4", "pde4"))):
        for m in models:
            assert any(rc.omega == 1.0 for rc in cases if rc.case.model == m), m
            assert cases is sm.RANGE_RBP or any(rc.omega != 1.0 for rc in cases if rc.case.model == m), m
    assert {(rc.case.nrows, rc.case.ncols) for rc in sm.RANGE_SMALL} == {(37, 53), (131, 70)} and {rc.case.it for rc in sm.RANGE_SMALL} == {4, 9}
    for m in ("elin4", "llin4", "disp4", "dispsym4", "pde4", "pde8"):
        mine = [rc.case for rc in sm.RANGE_RB if rc.case.model == m]
        assert {(c.tj, c.it) for c in mine} == {(t, i) for t in (3, 13) for i in (1, 2, 3)} and {(c.nrows, c.ncols) for c in mine} == {(252, 51), (8, 139)}
    for m in ("elin4", "llin4"):
        mine = [rc.case for rc in sm.RANGE_RBP if rc.case.model == m and rc.div_frac == sm.RANGE_MIXED]
        assert {(c.nrows, c.ncols, c.tj, c.it) for c in mine} == {(r, c, t, i) for r, c in ((244, 300), (484, 57)) for t in (9, 33) for i in (4, 9)}
        assert {c.serp for c in mine} == {0, 1, 2} and {c.inplace for c in mine} == {True, False} and {c.col0 for c in mine} == {0, 1}
    big = [rc.case for rc in sm.RANGE_RBP if rc.case.group == "B"]
    assert all(c.nrows * c.ncols == sm.PIPE_MIN_PIXELS and c.tj for c in big)
    assert ("pde4", 3) in {(c.model, c.nframes) for c in big} and ("disp4", 1) in {(c.model, c.serp) for c in big}
    for cases in (sm.RANGE_SMALL, sm.RANGE_RB, sm.RANGE_RBP):  # class T reaches every family, for every model it runs
        assert {rc.case.model for rc in cases if rc.corner} == {rc.case.model for rc in cases}
    assert all(rc.corner for rc in sm.RANGE_RBP if rc.div_frac == sm.RANGE_MIXED and rc.case.nrows * rc.case.ncols == sm.PIPE_MIN_PIXELS)
    # exact-order line relaxation: (7, 5200) is where a coupled model's row pass leaves the two-chain launch
    assert sm.alr_exact_launches("elin4", 131, 70, 3) == 1 + 2 + 3 * 4 and sm.alr_exact_launches("elin4", 7, 5200, 3) == 1 + 2 + 3 * 5
    assert sm.alr_exact_launches("disp4", 7, 5200, 1) == 1 + 2 + 4 and sm.alr_exact_launches("pde8", 37, 53, 3) == 1 + 2 + 4
    assert sm.exact_launches("elin4", 244, 300, 4, "persist") == 3 and sm.exact_launches("dispsym4", 37, 53, 1, "walk") == 6
    assert sm.exact_launches("elin4", 244, 300, 4, "front") == 1 + (4 + 2 * 4 + 3 * 3 + 1) + 1
