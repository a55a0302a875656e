"""CPU: the oracle's gateway wrappers (oracle_lib) bit for bit against the reference's own gateways.

The reference's mexFunctions are built unchanged into oracle/_ref/ (oracle/build_ref.py, against the stand-in MEX runtime
oracle/refmex/) and called through tests/ref_lib.py exactly as MATLAB calls them: MATLAB-shaped single arrays, single
scalars, nlhs.  Every comparison is in the reference's own (lexicographic) order.  The committed golden vectors and the
level-set restatements are replayed through the same build, so they are pinned to the reference, not only to the oracle.

Reinit is the one gateway that is not compared bit for bit: its sign function uses `rsqrtps`, a 12-bit estimate, and its
scalar tail reads an uninitialised register when rows*cols*frames % 4 != 0.  It is compared with a
float64 statement of the same step, within the bound rsqrtps's error allows, on sizes that are multiples of four.
"""
import importlib.util
import os

import numpy as np
import pytest

import cv_ref
import golden_util as gu
import levelset_ref as lr
import oracle_lib as orc
import problems as pb
import ref_lib

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_ref_module():
    spec = importlib.util.spec_from_file_location("pdeip_build_ref", os.path.join(ROOT, "oracle", "build_ref.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module", autouse=True)
def ref_build():
    """oracle/_ref/ must be there and current.  With a reference checkout at hand a missing or stale build is a failure;
    only when neither the checkout nor a build exists does the module skip."""
    br = _build_ref_module()
    tree = br.reference_dir()
    if tree is not None:
        if not br.up_to_date(tree):
            pytest.fail("oracle/_ref/ is missing or stale against the reference at %s: run `python __graft_entry__.py build` "
                        "(or oracle/build_ref.py)" % tree)
    elif ref_lib.available() is None:
        pytest.skip("no reference checkout and no oracle/_ref/ build: nothing to compare the oracle with")
    m = ref_lib.available()
    assert m is not None, "oracle/_ref/MANIFEST.json does not describe this tree's stand-in runtime"
    assert sorted(m["gateways"]) == sorted(br.GATEWAYS)
    return m


def same(got, want, what):
    """`got`: a gateway's outputs, trailing ones it never created (None) dropped, as MATLAB leaves them unassigned."""
    want = want if isinstance(want, tuple) else (want,)
    got = list(got)
    while got and got[-1] is None:
        got.pop()
    assert len(got) == len(want), "%s: %d outputs, want %d" % (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g is not None, "%s: output %d not created" % (what, k)
        assert g.shape == np.shape(w), "%s: output %d has dims %s, want %s" % (what, k, g.shape, np.shape(w))
        assert pb.bit_equal(g, w), "%s output %d: %s" % (what, k, pb.describe_mismatch(g, w))


# ---- the ordered gateways (SOR, solver 1 and 2) ------------------------------------------------------------------------------

SHAPES = [(3, 3), (4, 5), (5, 300), (260, 7), (131, 70), (97, 131), (388, 584)]
ITERS = [0, 1, 4, 7]
NANS = [("all", 0.05), ("C", 0.05), ("D", 0.05), ("all", 0.0)]
NLHS = {"Oflow_sor_elin4_2d": (2, 3, 4), "Oflow_sor_llin4_2d": (2, 3, 4), "Oflow_sor_llin8_2d": (2, 3, 4),
        "Disp_sor_llin4_2d": (1, 2), "Disp_sor_llin_sym4_2d": (2,), "PDEsolver4": (1,), "PDEsolver8": (1,)}
ORDERED = list(NLHS)


def problem(gw, seed, shape, frames, nan_mode, frac):
    r, c = shape
    if gw == "Oflow_sor_elin4_2d":
        return pb.elin4(seed, r, c, frames, frac, nan_mode)
    if gw == "Oflow_sor_llin4_2d":
        return pb.llin4(seed, r, c, frames, frac, nan_mode)
    if gw == "Oflow_sor_llin8_2d":
        return pb.llin8(seed, r, c, frames, frac)
    if gw == "Disp_sor_llin4_2d":
        return pb.disp4(seed, r, c, frac)
    if gw == "Disp_sor_llin_sym4_2d":
        return pb.dispsym4(seed, r, c, frac)
    if gw == "PDEsolver4":
        return pb.pde4(seed, r, c, frames, frac)
    return pb.pde8(seed, r, c, frames, frac)


def oracle_call(gw, p, it, omega, solver, nlhs):
    kw = {} if gw.startswith("PDE") else {"nargout": nlhs}
    return getattr(orc, gw)(*p.values(), it, omega, solver=solver, order=orc.LEX, **kw)


def ref_call(gw, p, it, omega, solver, nlhs):
    return ref_lib.call(gw, nlhs, *p.values(), F32(it), F32(omega), F32(solver))


def check_ordered(gw, p, it, omega, solver, nlhs, what):
    same(ref_call(gw, p, it, omega, solver, nlhs), oracle_call(gw, p, it, omega, solver, nlhs), what)


def matrix():
    """Every ordered gateway at every shape with both solvers; iter, frames, NaN lacing and nlhs rotate so each gateway
    meets every value of each with each solver."""
    cases = []
    for gi, gw in enumerate(ORDERED):
        for si, shape in enumerate(SHAPES):
            for solver in (1, 2):
                k = gi + si + solver
                nan_mode, frac = NANS[(gi + 2 * si + solver) % 4]
                cases.append((gw, shape, solver, ITERS[k % 4], 1 + k % 3, nan_mode, frac, NLHS[gw][k % len(NLHS[gw])],
                              1000 * gi + 10 * si + solver))
    return cases


def _id(c):
    gw, shape, solver, it, frames, nan_mode, frac, nlhs, _ = c
    return "%s-%dx%dx%d-s%d-it%d-%s%s-n%d" % (gw, shape[0], shape[1], frames, solver, it, nan_mode, frac, nlhs)


@pytest.mark.parametrize("case", matrix(), ids=_id)
def test_ordered_gateway_matches_the_reference(case):
    gw, shape, solver, it, frames, nan_mode, frac, nlhs, seed = case
    omega = 1.9 if solver == 1 else 1.4
    check_ordered(gw, problem(gw, seed, shape, frames, nan_mode, frac), it, omega, solver, nlhs, _id(case))


def test_matrix_covers_every_edge():
    cases = matrix()
    for gw in ORDERED:
        mine = [c for c in cases if c[0] == gw]
        for solver in (1, 2):
            assert {c[3] for c in mine if c[2] == solver} == set(ITERS)
        assert {c[7] for c in mine} == set(NLHS[gw])
        assert {c[1] for c in mine} == set(SHAPES)
        if gw.startswith("Oflow") or gw.startswith("PDE"):
            assert {c[4] for c in mine} == {1, 2, 3}
        if gw in ("Oflow_sor_elin4_2d", "Oflow_sor_llin4_2d"):
            assert {c[5] for c in mine if c[6] > 0} == {"all", "C", "D"}


@pytest.mark.parametrize("solver", [1, 2])
@pytest.mark.parametrize("gw", ["Oflow_sor_elin4_2d", "Oflow_sor_llin4_2d", "Oflow_sor_llin8_2d"])
def test_residual_outputs_of_multi_frame_data(gw, solver):
    """nlhs = 4 with 3-frame data terms: the residuals come back [nrows ncols nframes], with the :912 frame-0 quirk of
    Residuals_llin4_2d, and llin8's residual outputs are created but never filled."""
    p = problem(gw, 77, (19, 23), 3, "all", 0.05)
    got = ref_call(gw, p, 3, 1.7, solver, 4)
    assert got[2].shape == got[3].shape == (19, 23, 3)
    if gw == "Oflow_sor_llin8_2d":
        assert not got[2].any() and not got[3].any()
    same(got, oracle_call(gw, p, 3, 1.7, solver, 4), "%s solver %d" % (gw, solver))


def test_pde8_line_relaxation_ignores_iter():
    p = pb.pde8(31, 37, 41, 2, 0.03)
    one = ref_call("PDEsolver8", p, 1, 1.3, 2, 1)
    for it in (0, 4, 7):
        got = ref_call("PDEsolver8", p, it, 1.3, 2, 1)
        same(got, tuple(one), "PDEsolver8 solver 2 iter %d vs iter 1" % it)
        same(got, oracle_call("PDEsolver8", p, it, 1.3, 2, 1), "PDEsolver8 solver 2 iter %d" % it)


@pytest.mark.parametrize("shape", [(10300, 5), (6, 10290)], ids=["10300x5", "6x10290"])
@pytest.mark.parametrize("gw", ORDERED)
def test_line_relaxation_on_long_lines(gw, shape):
    """ALR lines longer than 5 120 and than 10 240 elements (the GPU line solver's chunk limits)."""
    check_ordered(gw, problem(gw, 55, shape, 2, "all", 0.02), 2, 1.4, 2, NLHS[gw][-1], "%s %s" % (gw, shape))


# ---- the pointwise gateways --------------------------------------------------------------------------------------------------

POINTWISE = ["Oflow_lhs_elin4_2d", "Oflow_lhs_llin4_2d", "DdiffWeights", "BilinInterp_2d", "FstDerivatives5", "SndDerivatives5"]
NOUT = {"Oflow_lhs_elin4_2d": 2, "Oflow_lhs_llin4_2d": 2, "DdiffWeights": 4, "BilinInterp_2d": 1, "FstDerivatives5": 3,
        "SndDerivatives5": 5}
LHS_KEYS = {"Oflow_lhs_elin4_2d": ("U", "V", "M", "Du", "Dv", "wW", "wN", "wE", "wS"),
            "Oflow_lhs_llin4_2d": ("U", "V", "dU", "dV", "M", "Du", "Dv", "wW", "wN", "wE", "wS")}


def pointwise_args(gw, seed, shape, frames):
    r, c = shape
    if gw == "Oflow_lhs_elin4_2d":
        p = pb.elin4(seed, r, c, frames, 0.05, "D")
        return [p[k] for k in LHS_KEYS[gw]]
    if gw == "Oflow_lhs_llin4_2d":
        p = pb.llin4(seed, r, c, frames, 0.05, "D")
        return [p[k] for k in LHS_KEYS[gw]]
    if gw == "DdiffWeights":
        return [pb.diffweights(seed, r, c, frames)["D"], F32(1e-3)]
    if gw == "BilinInterp_2d":
        w = pb.warp(seed, r, c, frames, max_disp=4.0, special=True)
        return [w["Iin"], w["X"], w["Y"]]
    ip = pb.image_pair(seed, r, c, frames)
    return [ip["It0"], ip["It1"]]


def pointwise_cases():
    """The derivative gateways meet 4x4 instead of 3x3: their 5-tap loops run `i < rows - 4` on unsigned ints, so the reference
    reads far outside any image narrower than 4 (imageDerivatives.c:92,164), where the library clamps."""
    def fit(gw, shape):
        return (4, 4) if gw.endswith("Derivatives5") and min(shape) < 4 else shape
    return [(gw, fit(gw, shape), 1 + (gi + si) % 3) for gi, gw in enumerate(POINTWISE) for si, shape in enumerate(SHAPES)]


def same_warp(got, want, what):
    """BilinInterp_2d: bit for bit wherever the library's result is a number.  Where it is NaN (coordinates out of range, or
    not finite) the reference holds NaN or its undefined fill: BilinInterp_2d.c:120 calls bilinInterp2 without a prototype
    and without its fifth parameter `NaN`, so the fill is whatever the first float argument register held (DESIGN.md
    section 2)."""
    assert len(got) == 1 and got[0].shape == want.shape, what
    g, nan = got[0], np.isnan(want)
    assert pb.bit_equal(g[~nan], want[~nan]), "%s: %s" % (what, pb.describe_mismatch(np.where(nan, 0, g), np.where(nan, 0, want)))


@pytest.mark.parametrize("case", pointwise_cases(), ids=lambda c: "%s-%dx%dx%d" % (c[0], c[1][0], c[1][1], c[2]))
def test_pointwise_gateway_matches_the_reference(case):
    gw, shape, frames = case
    args = pointwise_args(gw, 300 + frames, shape, frames)
    want = getattr(orc, gw)(*[float(a) if np.ndim(a) == 0 else a for a in args])
    what = "%s %s x%d" % (gw, shape, frames)
    if gw == "BilinInterp_2d":
        same_warp(ref_lib.call(gw, 1, *args), want, what)
    else:
        same(ref_lib.call(gw, NOUT[gw], *args), want, what)


def test_warp_coordinates_on_and_beyond_the_border():
    for shape, frames in (((6, 6), 1), ((9, 13), 3), ((64, 96), 2)):
        w = pb.warp(8, shape[0], shape[1], frames, special=True)
        want = orc.BilinInterp_2d(w["Iin"], w["X"], w["Y"])
        assert np.isnan(want).any() and not np.isnan(want).all()
        same_warp(ref_lib.call("BilinInterp_2d", 1, w["Iin"], w["X"], w["Y"]), want, "BilinInterp_2d %s x%d" % (shape, frames))


# ---- the golden vectors, replayed through the reference -----------------------------------------------------------------------

DEFAULT_NLHS = dict({gw: n[0] for gw, n in NLHS.items()}, **NOUT)


class _RefApi:
    """golden_util.call's `api`: gateway name -> the reference's gateway (single-precision scalars, as MATLAB passes)."""

    def __getattr__(self, gw):
        return lambda *args, nargout=DEFAULT_NLHS[gw]: ref_lib.call(gw, nargout, *args)


@pytest.mark.parametrize("name", gu.names())
def test_golden_vectors_are_the_references_outputs(name):
    meta, inputs, outs = gu.load(name)
    fn, args, kw = gu.call(_RefApi(), meta, inputs, single=True)
    want = outs["lex" if "lex" in outs else "any"]
    if meta["gateway"] == "BilinInterp_2d":
        same_warp(fn(*args, **kw), want[0], name)
    else:
        same(fn(*args, **kw), want, name)


def test_cv_fixture_is_reproduced_by_the_committed_recipe():
    """tests/golden/levelset/cv_solver.npz was made by an uncommitted build of the reference; the committed one agrees."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "levelset", "cv_solver.npz"))
    for name in z["names"]:
        PHI, D, DH, G, out = (np.asfortranarray(z["%s/%s" % (name, k)]) for k in ("PHI", "D", "DH", "GradNorm", "out"))
        tau, nu = z["%s/tau_nu" % name]
        same(ref_lib.call("CV_solver_2d", 1, PHI, D, DH, G, F32(tau), F32(nu)), out, "cv_solver.npz " + str(name))


# ---- level sets ---------------------------------------------------------------------------------------------------------------

def ls_problem(seed, shape, nan=True):
    rng = np.random.default_rng(seed)
    phi = rng.uniform(-3, 3, shape).astype(F32)
    d = rng.uniform(-1, 1, shape).astype(F32)
    g = rng.uniform(0.0, 1.5, shape).astype(F32)
    diff = rng.uniform(0.0, 2.0, shape).astype(F32)
    for a in (g, diff):
        a[rng.random(shape) < 0.05] = 0
        a[0, ...] = np.where(rng.random(a[0].shape) < 0.3, 0, a[0])
        a[-1, ...] = np.where(rng.random(a[-1].shape) < 0.3, 0, a[-1])
        a[:, 0] = np.where(rng.random(a[:, 0].shape) < 0.3, 0, a[:, 0])
        a[:, -1] = np.where(rng.random(a[:, -1].shape) < 0.3, 0, a[:, -1])
    if nan:
        d[rng.random(shape) < 0.02] = np.nan
    return [np.asfortranarray(x) for x in (phi, d, g, diff)]


def drivsco_problems():
    """Per drivsco image: the GAC drivers' first AOS step's inputs -- PHI the initial box (runme.m), GradNorm and Diff the
    stopping function g of the image, D = c*g (c = -0.1)."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "levelset", "drivsco.npz"))
    PHI = -np.ones((320, 400), F32, order="F")
    PHI[41:175, 114:217] = 1
    PHI = lr.Reinit(PHI, F32(10))
    probs = []
    for k in ("I1", "I2"):
        g = np.asfortranarray(lr.gac_stopping(np.asfortranarray(z[k].astype(F32) / F32(255)))[0].astype(F32))
        probs.append((k, PHI, np.asfortranarray(F32(-0.1) * g), g, g))
    return probs


LS_SHAPES = [(2, 2), (3, 5), (97, 61), (61, 97), (23, 17, 3), (3, 2048), (2048, 3)]


def _ls_id(s):
    return "x".join(map(str, s))


@pytest.mark.parametrize("shape", LS_SHAPES, ids=_ls_id)
def test_cv_solver_matches_the_restatement(shape):
    phi, d, dh, g = ls_problem(21, shape)
    for tau, nu in ((F32(0.25), F32(1.3)), (F32(1.0), F32(0.0))):
        same(ref_lib.call("CV_solver_2d", 1, phi, d, dh, g, tau, nu), cv_ref.CV_solver_2d(phi, d, dh, g, tau, nu),
             "CV_solver_2d %s tau %g nu %g" % (shape, tau, nu))


@pytest.mark.parametrize("img", [0, 1])
def test_level_set_steps_on_the_drivsco_images(img):
    name, PHI, D, G, Diff = drivsco_problems()[img]
    tau, nu = F32(0.25), F32(1.0)
    same(ref_lib.call("CV_solver_2d", 1, PHI, D, G, Diff, tau, nu), cv_ref.CV_solver_2d(PHI, D, G, Diff, tau, nu), "CV " + name)
    check_ac(PHI, D, G, Diff, tau, nu, "AC " + name)


def check_ac(phi, d, g, diff, tau, nu, what):
    """AC_AOS_4_2d = column pass, row pass, then reinit(PHI, 0.25f): the reference's own Reinit gateway with T = 0.25 runs the
    very same step.  So the passes are compared bit for bit through it (rsqrtps and all), and the whole step is within the
    rsqrtps bound of the float64 statement."""
    assert phi.size % 4 == 0
    passes = lr.aos_row(phi, d, g, diff, tau, nu, lr.aos_column(phi, d, g, diff, tau, nu))
    got = ref_lib.call("AC_solver_2d", 1, phi, d, g, diff, tau, nu)
    same(got, tuple(ref_lib.call("Reinit", 1, passes, F32(0.25))), what + ": passes (through the reference's reinit step)")
    within_rsqrt_bound(got[0], passes, what)


@pytest.mark.parametrize("nan", [False, True], ids=["finite", "nan"])
@pytest.mark.parametrize("shape", [(4, 5), (96, 60), (60, 96), (24, 17, 3), (4, 2048), (2048, 4)], ids=_ls_id)
def test_ac_solver_matches_the_restatement(shape, nan):
    phi, d, g, diff = ls_problem(11, shape, nan)
    check_ac(phi, d, g, diff, F32(0.25), F32(1.3), "AC_solver_2d %s" % (shape,))


# Reinit: the float64 statement and the bound rsqrtps allows ----------------------------------------------------------------------

EPS32 = 2.0 ** -24          # unit roundoff of float32
RSQRT_REL = 1.5 * 2.0 ** -12  # |rsqrtps(x) / (1/sqrt(x)) - 1| at most (Intel and AMD document this bound)


def reinit_step64(P):
    """One step of reinit() in float64 from the float32 input: returns (out, S, S*r), the same formulas as
    levelset_ref.reinit_step (the SSE branch), each operation exact to float64."""
    P3 = np.asarray(P, np.float64)
    P3 = P3 if P3.ndim == 3 else P3[:, :, None]
    nr, nc = P3.shape[:2]
    pN = np.concatenate([P3[:1], P3[:-1]], 0)
    pS = np.concatenate([P3[1:], P3[-1:]], 0)
    pW = np.concatenate([P3[:, :1], P3[:, :-1]], 1)
    pE = np.concatenate([P3[:, 1:], P3[:, -1:]], 1)
    gx, gy = 0.5 * (pE - pW), 0.5 * (pS - pN)
    m2 = np.sqrt(gx * gx + gy * gy + float(np.finfo(F32).eps))
    S = P3 / np.sqrt(m2 + P3 * P3)
    i = np.arange(nr)[:, None, None]
    j = np.arange(nc)[None, :, None]
    xfd, xbd = np.where(j < nc - 1, pE - P3, 0.0), np.where(j > 0, P3 - pW, 0.0)
    yfd, ybd = np.where(i < nr - 1, pS - P3, 0.0), np.where(i > 0, P3 - pN, 0.0)
    pos = S > 0

    def up(b, f):  # Godunov: the upwind one-sided difference squared
        return np.where(pos, np.maximum(np.maximum(b, 0) ** 2, np.minimum(f, 0) ** 2),
                        np.maximum(np.minimum(b, 0) ** 2, np.maximum(f, 0) ** 2))

    Sr = S * np.sqrt(up(xbd, xfd) + up(ybd, yfd))
    out = P3 + 0.25 * (S - Sr)
    return out.reshape(np.shape(P)), S.reshape(np.shape(P)), Sr.reshape(np.shape(P))


def rsqrt_bound(P):
    """|float32 step - float64 step| allowed, per pixel.  First-order error analysis of the float32 evaluation:
    the halved central differences carry eps each; |grad|^2 + FLT_EPSILON (4 eps), its sqrt (3 eps) and + PHI^2 leave m1 within
    5 eps; rsqrtps(m1) is within RSQRT_REL + 2.5 eps of 1/sqrt(m1) (a correctly rounded 1/sqrtf within 4.5 eps), and the
    multiply by PHI adds one more: S carries e_S = RSQRT_REL + 6 eps, the same factor on S and on S*r, so on S - S*r it costs
    |S - S*r| * e_S.  r = sqrt(X2 + Y2) carries 4 eps (one rounding in each one-sided difference, squares, sum, sqrt), the
    product S*r one more, the subtraction and the final + PHI one each (the 0.25 is exact).  A 2x factor covers the
    second-order terms and the Godunov maxima, which are 1-Lipschitz in their arguments."""
    out, S, Sr = reinit_step64(P)
    e_S = RSQRT_REL + 6 * EPS32
    b = 0.25 * (np.abs(S - Sr) * e_S + 6 * EPS32 * np.abs(Sr) + EPS32 * np.abs(S - Sr)) + EPS32 * np.abs(out)
    return out, 2.0 * b + np.spacing(np.abs(out).astype(F32)).astype(np.float64) * 0.5


def within_rsqrt_bound(got, P, what):
    """Asserts |got - float64 step| <= the bound wherever the float64 step is a number, and NaN exactly where it is NaN.
    Returns the largest error as a fraction of its bound."""
    out, bound = rsqrt_bound(P)
    assert np.array_equal(np.isnan(got), np.isnan(out)), "%s: NaN at other pixels than the float64 step's" % what
    err = np.abs(got.astype(np.float64) - out)
    bad = ~((err <= bound) | np.isnan(out))
    assert not bad.any(), "%s: %d pixels beyond the rsqrtps bound; worst error %.3g against a bound of %.3g" % (
        what, int(bad.sum()), float(np.nanmax(err)), float(bound.flat[int(np.nanargmax(err - bound))]))
    return float(np.nanmax(err / np.maximum(bound, 1e-300)))


REINIT_SHAPES = [(4, 5), (8, 8), (40, 60), (33, 24, 2), (320, 400), (2048, 4)]


@pytest.mark.parametrize("shape", REINIT_SHAPES, ids=_ls_id)
def test_reinit_within_the_rsqrt_bound(shape):
    assert int(np.prod(shape)) % 4 == 0  # the scalar tail reads an uninitialised register otherwise (section 5.7)
    rng = np.random.default_rng(12)
    phi = np.asfortranarray(rng.uniform(-4, 4, shape).astype(F32))
    outs, ins = ref_lib.call("Reinit", 1, phi, F32(0.25), return_inputs=True)
    got, after = outs[0], ins[0]
    assert pb.bit_equal(after, got)  # Reinit.c:136-137 runs the step in place on its input, then copies it out
    used = within_rsqrt_bound(got, phi, "Reinit %s" % (shape,))
    assert used > 0.01, "the reference's step agrees with float64 far inside the bound (%.3g of it): is rsqrtps still there?" % used
    within_rsqrt_bound(lr.reinit_step(phi), phi, "levelset_ref.reinit_step %s" % (shape,))


def test_the_rsqrt_bound_is_tight_enough_to_matter():
    """A step whose sign function lost one more bit than rsqrtps's (relative error 2^-11 on S) leaves the bound."""
    rng = np.random.default_rng(5)
    phi = np.asfortranarray(rng.uniform(-4, 4, (40, 60)).astype(F32))
    out, S, Sr = reinit_step64(phi)
    worse = (phi + 0.25 * (S - Sr) * (1 + 2.0 ** -10)).astype(F32)
    with pytest.raises(AssertionError):
        within_rsqrt_bound(worse, phi, "degraded sign function")


# ---- the stand-in runtime itself ----------------------------------------------------------------------------------------------

def test_stand_in_passes_dims_as_the_library_reads_them():
    """mwSize must be 32 bits: the library reads dims through `const unsigned int *` / `const int *`.  A 2x3x2 input must come
    back with the dims it went in with, and the values the library computed over them."""
    for gw in ref_lib.manifest()["gateways"]:
        assert ref_lib.mwsize_bytes(gw) == 4, gw
    w = pb.warp(3, 2, 3, 2, max_disp=0.4)
    got = ref_lib.call("BilinInterp_2d", 1, w["Iin"], w["X"], w["Y"])
    assert got[0].shape == (2, 3, 2)
    same_warp(got, orc.BilinInterp_2d(w["Iin"], w["X"], w["Y"]), "BilinInterp_2d 2x3x2")
    D = pb.diffweights(4, 2, 3, 2)["D"]
    got = ref_lib.call("DdiffWeights", 4, D, F32(1e-3))
    assert [g.shape for g in got] == [(2, 3, 2)] * 4
    same(got, orc.DdiffWeights(D, 1e-3), "DdiffWeights 2x3x2")
    p = pb.pde4(5, 2, 3, 2)
    same(ref_lib.call("PDEsolver4", 1, *p.values(), F32(2), F32(1.5), F32(1)), orc.PDEsolver4(*p.values(), 2, 1.5),
         "PDEsolver4 2x3x2")


def test_stand_in_reports_errors_and_class():
    p = pb.pde4(6, 5, 6)
    args = list(p.values()) + [F32(1), F32(1.5), F32(1)]
    with pytest.raises(ref_lib.RefMexError, match="wrong number of input parameters"):
        ref_lib.call("PDEsolver4", 1, *args[:-1])
    bad = list(args)
    bad[1] = bad[1].astype(np.float64)
    with pytest.raises(ref_lib.RefMexError, match="TRACE"):
        ref_lib.call("PDEsolver4", 1, *bad)
    same(ref_lib.call("PDEsolver4", 1, *args), orc.PDEsolver4(*p.values(), 1, 1.5), "PDEsolver4 after errors")


# ---- argument checks: every call the reference refuses, the drop-in stub refuses too --------------------------------------------

MIN_NLHS = dict({gw: n[0] for gw, n in NLHS.items()}, Oflow_lhs_elin4_2d=2, Oflow_lhs_llin4_2d=2, DdiffWeights=4,
                BilinInterp_2d=1, FstDerivatives5=3, SndDerivatives5=5, AC_solver_2d=1, CV_solver_2d=1, Reinit=1)
LEVEL_SET = ("AC_solver_2d", "CV_solver_2d", "Reinit")


def valid_args(gw):
    if gw in NLHS:
        return list(problem(gw, 9, (8, 9), 2, "all", 0.0).values()) + [F32(2), F32(1.5), F32(1)]
    if gw in POINTWISE:
        return pointwise_args(gw, 9, (8, 9), 2)
    phi, d, g, diff = ls_problem(9, (8, 9), nan=False)
    return [phi, F32(1)] if gw == "Reinit" else [phi, d, g, diff, F32(0.25), F32(1.0)]


def refused_calls(gw):
    """(label, nlhs, args) of the wrong calls: one argument short, one too many, each argument in double, one output short."""
    args, nlhs = valid_args(gw), MIN_NLHS[gw]
    yield "nrhs-1", nlhs, args[:-1]
    yield "nrhs+1", nlhs, args + [F32(0)]
    for k in range(len(args)):
        yield "double#%d" % k, nlhs, args[:k] + [np.asarray(args[k], np.float64)] + args[k + 1:]
    yield "nlhs-1", nlhs - 1, args


@pytest.mark.parametrize("gw", sorted(MIN_NLHS))
def test_stub_refuses_what_the_reference_refuses(pdeip, gw):
    from test_levelset import build_ls_stub
    from test_mex_stubs import build_stub, call

    stub = build_ls_stub(gw, pdeip) if gw in LEVEL_SET else build_stub(gw, pdeip)
    refused = 0
    for label, nlhs, args in refused_calls(gw):
        try:
            ref_lib.call(gw, nlhs, *args)
            continue  # the reference takes this call; the stub may or may not
        except ref_lib.RefMexError:
            refused += 1
        err, _ = call(stub, nlhs, args)
        assert err is not None, "%s %s: the reference refuses the call, the stub takes it" % (gw, label)
        assert "hip" not in err.lower() and "device" not in err.lower(), "%s %s: refused only by the GPU: %s" % (gw, label, err)
    assert refused >= 3, "%s: the reference refused only %d of the wrong calls" % (gw, refused)
