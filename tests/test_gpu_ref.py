"""GPU: the product in EXACT_ORDER bit for bit against the reference's own gateways (oracle/_ref/, see test_ref_oracle.py).

Each case is called through mex_api, and for every gateway at least once through its drop-in stub (built against
tests/mexmock as test_mex_stubs.py does) with the same MATLAB-shaped arguments.  RED_BLACK and zebra orders are not the
reference's and stay compared with the oracle's colour order elsewhere.  Reinit is compared with the float64 statement of
its step within the rsqrtps bound (test_ref_oracle.rsqrt_bound); the GPU stays bit-identical to levelset_ref.py, as
test_gpu_levelset.py already requires."""
import ctypes

import numpy as np
import pytest

import cv_ref
import levelset_ref as lr
import problems as pb
import ref_lib
from test_levelset import build_ls_stub
from test_mex_stubs import build_stub, call, to_mx
from test_ref_oracle import (LEVEL_SET, LS_SHAPES, MIN_NLHS, NLHS, NOUT, POINTWISE, _id, drivsco_problems, ls_problem, matrix,
                             pointwise_args, pointwise_cases, problem, same, same_warp, valid_args, within_rsqrt_bound)

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def ref_build(pdeip):
    if ref_lib.available() is None:
        import test_ref_oracle

        if test_ref_oracle._build_ref_module().reference_dir() is not None:
            pytest.fail("oracle/_ref/ is missing or stale: run `python __graft_entry__.py build`")
        pytest.skip("no oracle/_ref/ build in this tree: nothing to compare the GPU with")
    pdeip.mex_api.set_mode(pdeip.MODE_EXACT_ORDER)
    yield
    pdeip.mex_api.set_mode(pdeip.MODE_EXACT_ORDER)


def _tuple(x):
    return x if isinstance(x, tuple) else (x,)


def gpu_ordered(pdeip, gw, p, it, omega, solver, nlhs):
    return _tuple(getattr(pdeip.mex_api, gw)(*p.values(), F32(it), F32(omega), F32(solver), nargout=nlhs))


def ref_ordered(gw, p, it, omega, solver, nlhs):
    return ref_lib.call(gw, nlhs, *p.values(), F32(it), F32(omega), F32(solver))


def check_ordered(pdeip, gw, p, it, omega, solver, nlhs, what):
    same(ref_ordered(gw, p, it, omega, solver, nlhs), gpu_ordered(pdeip, gw, p, it, omega, solver, nlhs), what)


@pytest.mark.parametrize("case", matrix(), ids=_id)
def test_ordered_gateway_matches_the_reference(pdeip, case):
    gw, shape, solver, it, frames, nan_mode, frac, nlhs, seed = case
    omega = 1.9 if solver == 1 else 1.4
    check_ordered(pdeip, gw, problem(gw, seed, shape, frames, nan_mode, frac), it, omega, solver, nlhs, _id(case))


@pytest.mark.parametrize("shape", [(10300, 5), (6, 10290)], ids=["10300x5", "6x10290"])
@pytest.mark.parametrize("gw", list(NLHS))
def test_line_relaxation_on_long_lines(pdeip, gw, shape):
    check_ordered(pdeip, gw, problem(gw, 55, shape, 2, "all", 0.02), 2, 1.4, 2, NLHS[gw][-1], "%s %s" % (gw, shape))


@pytest.mark.parametrize("case", pointwise_cases(), ids=lambda c: "%s-%dx%dx%d" % (c[0], c[1][0], c[1][1], c[2]))
def test_pointwise_gateway_matches_the_reference(pdeip, case):
    gw, shape, frames = case
    args = pointwise_args(gw, 300 + frames, shape, frames)
    got = _tuple(getattr(pdeip.mex_api, gw)(*args))
    what = "%s %s x%d" % (gw, shape, frames)
    if gw == "BilinInterp_2d":
        same_warp(ref_lib.call(gw, 1, *args), got[0], what)
    else:
        same(ref_lib.call(gw, NOUT[gw], *args), got, what)


@pytest.mark.parametrize("gw", sorted(MIN_NLHS))
def test_stub_matches_the_reference(pdeip, gw):
    """One call per gateway through the drop-in stub, with the arguments MATLAB would pass."""
    stub = build_ls_stub(gw, pdeip) if gw in LEVEL_SET else build_stub(gw, pdeip)
    args = valid_args(gw)
    nlhs = max(NLHS.get(gw, (NOUT.get(gw, 1),)))
    if gw in NLHS:
        p = problem(gw, 19, (37, 45), 2, "all", 0.03)
        args = list(p.values()) + [F32(3), F32(1.6), F32(2 if gw.startswith("PDE") else 1)]
    err, outs = call(stub, nlhs, args)
    assert err is None, err
    want = ref_lib.call(gw, nlhs, *args)
    if gw == "BilinInterp_2d":
        same_warp(want, outs[0], "stub " + gw)
    elif gw in ("AC_solver_2d", "Reinit"):  # the reference's sign function is rsqrtps: not the contract
        phi = args[0]
        lr_want = lr.Reinit(phi, args[1]) if gw == "Reinit" else lr.AC_solver_2d(*args)
        same(outs, (lr_want,), "stub " + gw + " vs levelset_ref")
    else:
        same(want, tuple(outs), "stub " + gw)


# ---- full size (the C1-C5 shapes of test_gpu_fullsize.py) ------------------------------------------------------------------------

def test_c1_horn_schunck_388x584_iter20(pdeip):
    check_ordered(pdeip, "Oflow_sor_elin4_2d", pb.elin4(701, 388, 584), 20, 1.9, 1, 4, "C1 elin4")


def test_c2_late_linearization_1080x1920(pdeip):
    check_ordered(pdeip, "Oflow_sor_llin4_2d", pb.llin4(702, 1080, 1920, nan_frac=0.01), 4, 1.9, 1, 4, "C2 llin4")
    w = pb.warp(703, 1080, 1920, nframes=6, special=True)
    same_warp(ref_lib.call("BilinInterp_2d", 1, w["Iin"], w["X"], w["Y"]), pdeip.mex_api.BilinInterp_2d(w["Iin"], w["X"], w["Y"]),
              "C2 warp C=6")


def test_c3_tv8_2160x3840(pdeip):
    check_ordered(pdeip, "PDEsolver8", pb.pde8(704, 2160, 3840, nan_frac=0.001), 4, 1.75, 1, 1, "C3 pde8")


def test_c4_elin_fmg_smoother_2160x3840(pdeip):
    p = pb.elin4(705, 2160, 3840)
    check_ordered(pdeip, "Oflow_sor_elin4_2d", p, 4, 1.9, 1, 4, "C4 elin4 + residuals")
    args = [p[k] for k in ("U", "V", "M", "Du", "Dv", "wW", "wN", "wE", "wS")]
    same(ref_lib.call("Oflow_lhs_elin4_2d", 2, *args), pdeip.mex_api.Oflow_lhs_elin4_2d(*args), "C4 lhs")


def test_c5_disparity_1988x2880(pdeip):
    check_ordered(pdeip, "Disp_sor_llin4_2d", pb.disp4(706, 1988, 2880, nan_frac=0.01), 4, 1.9, 1, 2, "C5 disp")
    d = pb.diffweights(707, 1988, 2880)
    same(ref_lib.call("DdiffWeights", 4, d["D"], F32(1e-5)), pdeip.mex_api.DdiffWeights(d["D"], F32(1e-5)), "C5 diffweights")


def test_line_relaxation_at_config_sizes(pdeip):
    check_ordered(pdeip, "Oflow_sor_llin4_2d", pb.llin4(711, 1080, 1920, nan_frac=0.01), 2, 1.5, 2, 2, "C2 llin4 ALR")
    check_ordered(pdeip, "PDEsolver8", pb.pde8(712, 1080, 1920, nan_frac=0.001), 4, 1.3, 2, 1, "C3-shaped pde8 ALR")
    check_ordered(pdeip, "Disp_sor_llin4_2d", pb.disp4(713, 1988, 2880, nan_frac=0.01), 1, 1.5, 2, 1, "C5 disparity ALR")


# ---- level sets ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", LS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cv_solver_matches_the_reference(pdeip, shape):
    phi, d, dh, g = ls_problem(21, shape)
    for tau, nu in ((F32(0.25), F32(1.3)), (F32(1.0), F32(0.0))):
        want = ref_lib.call("CV_solver_2d", 1, phi, d, dh, g, tau, nu)
        same(want, (pdeip.mex_api.CV_solver_2d(phi, d, dh, g, tau, nu),), "CV_solver_2d %s tau %g nu %g" % (shape, tau, nu))


@pytest.mark.parametrize("img", [0, 1])
def test_level_set_steps_on_the_drivsco_images(pdeip, img):
    name, PHI, D, G, Diff = drivsco_problems()[img]
    tau, nu = F32(0.25), F32(1.0)
    same(ref_lib.call("CV_solver_2d", 1, PHI, D, G, Diff, tau, nu), (pdeip.mex_api.CV_solver_2d(PHI, D, G, Diff, tau, nu),),
         "CV " + name)
    check_ac_gpu(pdeip, PHI, D, G, Diff, tau, nu, "AC " + name)


def check_ac_gpu(pdeip, phi, d, g, diff, tau, nu, what):
    """The GPU's AC step: bit for bit the restatement (the contract), and within the rsqrtps bound of the float64 step on the
    passes -- where the reference's own step also lies (test_ref_oracle.check_ac)."""
    got = pdeip.mex_api.AC_solver_2d(phi, d, g, diff, tau, nu)
    same((got,), lr.AC_solver_2d(phi, d, g, diff, tau, nu), what + " vs levelset_ref")
    passes = lr.aos_row(phi, d, g, diff, tau, nu, lr.aos_column(phi, d, g, diff, tau, nu))
    within_rsqrt_bound(got, passes, what + " (GPU)")
    if phi.size % 4 == 0:
        within_rsqrt_bound(ref_lib.call("AC_solver_2d", 1, phi, d, g, diff, tau, nu)[0], passes, what + " (reference)")


@pytest.mark.parametrize("nan", [False, True], ids=["finite", "nan"])
@pytest.mark.parametrize("shape", [(4, 5), (96, 60), (24, 17, 3), (2048, 4), (7, 9)], ids=lambda s: "x".join(map(str, s)))
def test_ac_solver_within_the_reference_bound(pdeip, shape, nan):
    phi, d, g, diff = ls_problem(11, shape, nan)
    check_ac_gpu(pdeip, phi, d, g, diff, F32(0.25), F32(1.3), "AC_solver_2d %s" % (shape,))


@pytest.mark.parametrize("shape", [(4, 5), (40, 60), (33, 24, 2), (320, 400), (2048, 4)], ids=lambda s: "x".join(map(str, s)))
def test_reinit_within_the_rsqrt_bound(pdeip, shape):
    rng = np.random.default_rng(12)
    phi = np.asfortranarray(rng.uniform(-4, 4, shape).astype(F32))
    keep = phi.copy()
    got = pdeip.mex_api.Reinit(phi, F32(0.25))
    assert pb.bit_equal(phi, keep)
    same((got,), lr.Reinit(phi, F32(0.25)), "Reinit %s vs levelset_ref" % (shape,))
    within_rsqrt_bound(got, phi, "Reinit %s (GPU)" % (shape,))
    within_rsqrt_bound(ref_lib.call("Reinit", 1, phi, F32(0.25))[0], phi, "Reinit %s (reference)" % (shape,))


def test_reinit_input_modified_by_the_reference_not_by_the_stub(pdeip):
    """Reinit.c:136-137 runs the steps in place on its input and copies the result out; the stub leaves the input alone."""
    rng = np.random.default_rng(13)
    phi = np.asfortranarray(rng.uniform(-4, 4, (24, 20)).astype(F32))
    outs, ins = ref_lib.call("Reinit", 1, phi, F32(2), return_inputs=True)
    assert not pb.bit_equal(ins[0], phi) and pb.bit_equal(ins[0], outs[0])
    lib = build_ls_stub("Reinit", pdeip)
    prhs = (ctypes.c_void_p * 2)(to_mx(lib, phi), to_mx(lib, F32(2)))
    plhs = (ctypes.c_void_p * 1)()
    try:
        assert lib.mock_call(1, plhs, 2, prhs) == 0, lib.mock_last_error().decode()
        after = np.ctypeslib.as_array(ctypes.cast(lib.mock_data(prhs[0]), ctypes.POINTER(ctypes.c_float)), shape=(phi.size,))
        assert pb.bit_equal(after.reshape(phi.shape, order="F"), phi)
        out = np.ctypeslib.as_array(ctypes.cast(lib.mock_data(plhs[0]), ctypes.POINTER(ctypes.c_float)), shape=(phi.size,))
        assert pb.bit_equal(out.reshape(phi.shape, order="F"), lr.Reinit(phi, F32(2)))
    finally:
        for p in list(prhs) + list(plhs):
            if p:
                lib.mock_free(p)


def test_no_persistent_error(pdeip):
    assert pdeip.capi.load().pdeip_persist_error() == 0
