"""GPU parity: every gateway of the hot path, through the C-ABI, against the CPU oracle on the
same seeded inputs.  Bar: bit-exact (float32 arithmetic in the reference's operation order).

EXACT_ORDER mode is compared with the oracle's lexicographic (reference) order; RED_BLACK mode
with the oracle's colour order (same per-pixel arithmetic, red-black / four-colour sweeps).
"""
import os

import numpy as np
import pytest

import problems as pb

pytestmark = pytest.mark.gpu

SIZES = [(32, 48), (97, 131), (64, 200), (131, 70), (3, 3), (5, 300), (260, 7), (388, 584)]
MODES = [(0, 0), (1, 1)]  # (product mode, oracle order)


def check(got, want, what):
    got = got if isinstance(got, tuple) else (got,)
    want = want if isinstance(want, tuple) else (want,)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert pb.bit_equal(g, w), "%s output %d: %s" % (what, k, pb.describe_mismatch(g, w))


@pytest.mark.parametrize("mode,order", MODES)
@pytest.mark.parametrize("shape", SIZES)
@pytest.mark.parametrize("it", [1, 4, 7])
def test_oflow_sor_elin4(pdeip, oracle, mode, order, shape, it):
    p = pb.elin4(11, *shape)
    pdeip.mex_api.set_mode(mode)
    got = pdeip.mex_api.Oflow_sor_elin4_2d(*p.values(), np.float32(it), np.float32(1.9), np.float32(1))
    want = oracle.Oflow_sor_elin4_2d(*p.values(), it, 1.9, order=order)
    check(got, want, "elin4 %s it=%d mode=%d" % (shape, it, mode))


@pytest.mark.parametrize("mode,order", MODES)
def test_oflow_sor_elin4_nan_frames_residuals(pdeip, oracle, mode, order):
    pdeip.mex_api.set_mode(mode)
    for nan_mode in ("all", "C", "D"):
        p = pb.elin4(12, 97, 131, nframes=3, nan_frac=0.05, nan_mode=nan_mode)
        got = pdeip.mex_api.Oflow_sor_elin4_2d(*p.values(), np.float32(5), np.float32(1.7), np.float32(1), nargout=4)
        want = oracle.Oflow_sor_elin4_2d(*p.values(), 5, 1.7, nargout=4, order=order)
        check(got, want, "elin4 nan=%s mode=%d" % (nan_mode, mode))
    # iter = 0: zero iterate outputs, residuals of the input (FMG driver usage)
    p = pb.elin4(13, 64, 48, nframes=2)
    got = pdeip.mex_api.Oflow_sor_elin4_2d(*p.values(), np.float32(0), np.float32(1.9), np.float32(1), nargout=4)
    want = oracle.Oflow_sor_elin4_2d(*p.values(), 0, 1.9, nargout=4, order=order)
    check(got, want, "elin4 iter=0")
    assert not got[0].any() and not got[1].any()


@pytest.mark.parametrize("mode,order", MODES)
@pytest.mark.parametrize("shape", SIZES)
def test_oflow_sor_llin4(pdeip, oracle, mode, order, shape):
    pdeip.mex_api.set_mode(mode)
    for it, nan_frac in ((1, 0.0), (4, 0.04)):
        p = pb.llin4(21, *shape, nan_frac=nan_frac)
        got = pdeip.mex_api.Oflow_sor_llin4_2d(*p.values(), np.float32(it), np.float32(1.9), np.float32(1), nargout=4)
        want = oracle.Oflow_sor_llin4_2d(*p.values(), it, 1.9, nargout=4, order=order)
        check(got, want, "llin4 %s it=%d mode=%d" % (shape, it, mode))


@pytest.mark.parametrize("mode,order", MODES)
def test_oflow_sor_llin4_frames_quirk(pdeip, oracle, mode, order):
    """Multi-frame residuals incl. the frame-0 west-border quirk of Residuals_llin4_2d (:912)."""
    pdeip.mex_api.set_mode(mode)
    p = pb.llin4(22, 50, 37, nframes=3, nan_frac=0.03)
    got = pdeip.mex_api.Oflow_sor_llin4_2d(*p.values(), np.float32(3), np.float32(1.5), np.float32(1), nargout=4)
    want = oracle.Oflow_sor_llin4_2d(*p.values(), 3, 1.5, nargout=4, order=order)
    check(got, want, "llin4 frames")


@pytest.mark.parametrize("mode,order", MODES)
def test_oflow_sor_llin8(pdeip, oracle, mode, order):
    pdeip.mex_api.set_mode(mode)
    p = pb.llin8(23, 97, 131, nan_frac=0.02)
    got = pdeip.mex_api.Oflow_sor_llin8_2d(*p.values(), np.float32(4), np.float32(1.9), np.float32(1), nargout=4)
    want = oracle.Oflow_sor_llin8_2d(*p.values(), 4, 1.9, nargout=4, order=order)
    check(got, want, "llin8")
    assert not got[2].any() and not got[3].any()  # residual outputs are never filled by the gateway


def test_oflow_lhs(pdeip, oracle):
    for shape, F in (((97, 131), 1), ((40, 56), 3), ((3, 3), 1)):
        p = pb.elin4(31, *shape, nframes=F, nan_frac=0.05, nan_mode="D")
        args = [p[k] for k in ("U", "V", "M", "Du", "Dv", "wW", "wN", "wE", "wS")]
        check(pdeip.mex_api.Oflow_lhs_elin4_2d(*args), oracle.oflow_lhs_elin4(*args), "lhs_elin4 %s F=%d" % (shape, F))
        q = pb.llin4(32, *shape, nframes=F, nan_frac=0.05, nan_mode="D")
        args = [q[k] for k in ("U", "V", "dU", "dV", "M", "Du", "Dv", "wW", "wN", "wE", "wS")]
        check(pdeip.mex_api.Oflow_lhs_llin4_2d(*args), oracle.oflow_lhs_llin4(*args), "lhs_llin4 %s F=%d" % (shape, F))


@pytest.mark.parametrize("mode,order", MODES)
@pytest.mark.parametrize("shape", SIZES)
def test_disp_sor_llin4(pdeip, oracle, mode, order, shape):
    pdeip.mex_api.set_mode(mode)
    for it, nan_frac in ((1, 0.0), (6, 0.05)):
        p = pb.disp4(41, *shape, nan_frac=nan_frac)
        got = pdeip.mex_api.Disp_sor_llin4_2d(*p.values(), np.float32(it), np.float32(1.9), np.float32(1), nargout=2)
        want = oracle.Disp_sor_llin4_2d(*p.values(), it, 1.9, nargout=2, order=order)
        check(got, want, "disp %s it=%d mode=%d" % (shape, it, mode))


@pytest.mark.parametrize("mode,order", MODES)
@pytest.mark.parametrize("shape,F", [((32, 48), 1), ((97, 131), 3), ((3, 3), 1), ((260, 7), 2), ((64, 200), 1)])
def test_pde_sor4(pdeip, oracle, mode, order, shape, F):
    pdeip.mex_api.set_mode(mode)
    for it, nan_frac in ((1, 0.0), (5, 0.05), (0, 0.0)):
        p = pb.pde4(51, *shape, nframes=F, nan_frac=nan_frac)
        got = pdeip.mex_api.PDEsolver4(*p.values(), np.float32(it), np.float32(1.75), np.float32(1))
        want = oracle.PDEsolver4(*p.values(), it, 1.75, order=order)
        check(got, want, "pde4 %s F=%d it=%d mode=%d" % (shape, F, it, mode))


@pytest.mark.parametrize("mode,order", MODES)
@pytest.mark.parametrize("shape,F", [((32, 48), 1), ((97, 131), 3), ((3, 3), 1), ((260, 7), 2), ((5, 300), 1),
                                     ((64, 200), 1), ((200, 190), 1)])
def test_pde_sor8(pdeip, oracle, mode, order, shape, F):
    pdeip.mex_api.set_mode(mode)
    for it, nan_frac in ((1, 0.0), (2, 0.0), (5, 0.05), (0, 0.0)):
        p = pb.pde8(61, *shape, nframes=F, nan_frac=nan_frac)
        got = pdeip.mex_api.PDEsolver8(*p.values(), np.float32(it), np.float32(1.75), np.float32(1))
        want = oracle.PDEsolver8(*p.values(), it, 1.75, order=order)
        check(got, want, "pde8 %s F=%d it=%d mode=%d" % (shape, F, it, mode))


@pytest.mark.parametrize("shape,F,it", [((40, 330), 2, 3), ((300, 140), 1, 9), ((3, 70), 1, 2), ((130, 66), 1, 4), ((17, 129), 3, 6)])
def test_pde_sor8_exact_one_launch_vs_fronts(pdeip, oracle, shape, F, it):
    """Reference order, 9-point: the strip walkers (k_pde8_exact_persist, one launch) and the launch-per-front tiles give the
    oracle's bits -- several strips, a last strip of one column, more sweeps than strips, several frames."""
    pdeip.mex_api.set_mode(0)
    p = pb.pde8(67, *shape, nframes=F)
    want = oracle.PDEsolver8(*p.values(), it, 1.75, order=0)
    try:
        for knob in ("1", "0"):
            os.environ["PDEIP_PDE8_PERSIST"] = knob
            got = pdeip.mex_api.PDEsolver8(*p.values(), np.float32(it), np.float32(1.75), np.float32(1))
            check(got, want, "pde8 %s F=%d it=%d persist=%s" % (shape, F, it, knob))
    finally:
        os.environ.pop("PDEIP_PDE8_PERSIST", None)
    assert pdeip.capi.load().pdeip_persist_error() == 0


@pytest.mark.parametrize("shape,F", [((32, 48), 1), ((97, 131), 3), ((3, 3), 2), ((260, 7), 1), ((388, 584), 1)])
def test_diffweights(pdeip, oracle, shape, F):
    p = pb.diffweights(71, *shape, nframes=F)
    check(pdeip.mex_api.DdiffWeights(p["D"], np.float32(1e-5)), oracle.DdiffWeights(p["D"], 1e-5), "diffweights %s F=%d" % (shape, F))


@pytest.mark.parametrize("shape,F", [((32, 48), 1), ((97, 131), 3), ((6, 6), 2), ((388, 584), 6)])
def test_warp(pdeip, oracle, shape, F):
    p = pb.warp(81, *shape, nframes=F)
    check(pdeip.mex_api.BilinInterp_2d(p["Iin"], p["X"], p["Y"]), oracle.BilinInterp_2d(p["Iin"], p["X"], p["Y"]),
          "warp %s F=%d" % (shape, F))


@pytest.mark.parametrize("shape,F", [((32, 48), 1), ((97, 131), 3), ((4, 4), 2), ((5, 300), 1), ((260, 7), 1), ((388, 584), 2)])
def test_simoncelli_derivatives(pdeip, oracle, shape, F):
    p = pb.image_pair(85, *shape, nframes=F)
    check(pdeip.mex_api.FstDerivatives5(p["It0"], p["It1"]), oracle.FstDerivatives5(p["It0"], p["It1"]), "fst %s F=%d" % (shape, F))
    check(pdeip.mex_api.SndDerivatives5(p["It0"], p["It1"]), oracle.SndDerivatives5(p["It0"], p["It1"]), "snd %s F=%d" % (shape, F))


@pytest.mark.parametrize("mode,order", MODES)
@pytest.mark.parametrize("shape", [(32, 48), (97, 131), (3, 3), (260, 7), (388, 584)])
def test_disp_sor_llin_sym4(pdeip, oracle, mode, order, shape):
    pdeip.mex_api.set_mode(mode)
    for it, nan_frac, solver in ((1, 0.0, 1), (5, 0.04, 1), (0, 0.0, 1), (2, 0.03, 2)):
        p = pb.dispsym4(61, *shape, nan_frac=nan_frac)
        got = pdeip.mex_api.Disp_sor_llin_sym4_2d(*p.values(), np.float32(it), np.float32(1.7), np.float32(solver))
        want = oracle.Disp_sor_llin_sym4_2d(*p.values(), it, 1.7, solver=solver, order=order)
        check(got, want, "dispsym4 %s it=%d solver=%d mode=%d" % (shape, it, solver, mode))
    # not the plain disparity solver: omega multiplies the finished quotient here
    p = pb.dispsym4(62, *shape)
    a = pdeip.mex_api.Disp_sor_llin_sym4_2d(*p.values(), np.float32(3), np.float32(1.7), np.float32(1))[0]
    b = pdeip.mex_api.Disp_sor_llin4_2d(*list(p.values())[:8], np.float32(3), np.float32(1.7), np.float32(1))
    assert np.allclose(a, b, rtol=1e-4, atol=1e-5)


def test_solver_errors(pdeip):
    p = pb.elin4(91, 16, 16)
    with pytest.raises(pdeip.mex_api.MexError, match="no such solver"):
        pdeip.mex_api.Oflow_sor_elin4_2d(*p.values(), np.float32(1), np.float32(1.9), np.float32(7))
    q = pb.pde4(92, 16, 16)
    with pytest.raises(pdeip.mex_api.MexError, match="no such solver"):
        pdeip.mex_api.PDEsolver4(*q.values(), np.float32(1), np.float32(1.9), np.float32(3))


@pytest.mark.parametrize("shape", [(64, 80), (97, 131), (480, 300)])
@pytest.mark.parametrize("it", [0, 1, 2, 4, 5, 8, 9])
def test_out_of_place_elin4(pdeip, oracle, shape, it):
    """pdeip_oflow_sor_elin4_dev_to: the iterate is only read, the result lands in the second plane set -- both orderings,
    every launch-count parity of the red-black chain (1 / 2 / 4 sweeps per launch), vs the oracle and vs the in-place call."""
    import importlib

    dev, capi = importlib.import_module("pde-based-image-processing_amd.device"), pdeip.capi
    p = pb.elin4(901, *shape, nan_frac=0.01)
    coef = [dev.to_device(p[k]) for k in ("M", "Cu", "Cv", "Du", "Dv", "wW", "wN", "wE", "wS")]
    for mode, order in ((capi.MODE_RED_BLACK, oracle.COLOUR), (capi.MODE_EXACT_ORDER, oracle.LEX)):
        U, V = dev.to_device(p["U"]), dev.to_device(p["V"])
        U2, V2 = U.clone().fill_(7.0), V.clone().fill_(7.0)
        dev.oflow_sor_elin4(U, V, *coef, it, 1.9, mode, out=(U2, V2))
        want = oracle.oflow_sor_elin4(*p.values(), it, 1.9, order) if it > 0 else (p["U"], p["V"])
        assert pb.bit_equal(dev.to_matlab(U), p["U"]) and pb.bit_equal(dev.to_matlab(V), p["V"]), "the input planes were written"
        assert pb.bit_equal(dev.to_matlab(U2), want[0]), pb.describe_mismatch(dev.to_matlab(U2), want[0])
        assert pb.bit_equal(dev.to_matlab(V2), want[1])
        if it > 0:
            dev.oflow_sor_elin4(U, V, *coef, it, 1.9, mode)
            assert pb.bit_equal(dev.to_matlab(U), want[0]) and pb.bit_equal(dev.to_matlab(V), want[1])


def test_out_of_place_other_models(pdeip, oracle):
    """The llin4 / disp4 / pde4 out-of-place entry points through the C-ABI (device pointers), red-black, iter = 4 and 6."""
    import torch

    import importlib

    dev, capi = importlib.import_module("pde-based-image-processing_amd.device"), pdeip.capi
    st = lambda: torch.cuda.current_stream().cuda_stream
    for it in (4, 6):
        q = pb.llin4(902, 120, 96, nan_frac=0.02)
        d = {k: dev.to_device(v) for k, v in q.items()}
        o0, o1 = torch.empty_like(d["dU"]), torch.empty_like(d["dV"])
        capi.call("pdeip_oflow_sor_llin4_dev_to", st(), *[d[k].data_ptr() for k in ("U", "V", "dU", "dV")], o0.data_ptr(), o1.data_ptr(),
                  *[d[k].data_ptr() for k in ("M", "Cu", "Cv", "Du", "Dv", "wW", "wN", "wE", "wS")], 120, 96, it, 1.9, 1, 0)
        want = oracle.oflow_sor_llin4(*q.values(), it, 1.9, oracle.COLOUR)
        assert pb.bit_equal(dev.to_matlab(o0), want[0]) and pb.bit_equal(dev.to_matlab(o1), want[1])
        assert pb.bit_equal(dev.to_matlab(d["dU"]), q["dU"])
        e = pb.disp4(903, 120, 96, nan_frac=0.02)
        d = {k: dev.to_device(v) for k, v in e.items()}
        o = torch.empty_like(d["dU"])
        capi.call("pdeip_disp_sor_llin4_dev_to", st(), d["U"].data_ptr(), d["dU"].data_ptr(), o.data_ptr(),
                  *[d[k].data_ptr() for k in ("Cu", "Du", "wW", "wN", "wE", "wS")], 120, 96, it, 1.9, 1, 0)
        assert pb.bit_equal(dev.to_matlab(o), oracle.disp_sor_llin4(*e.values(), it, 1.9, oracle.COLOUR))
        f = pb.pde4(904, 120, 96, nframes=2, nan_frac=0.02)
        d = {k: dev.to_device(v) for k, v in f.items()}
        o = torch.empty_like(d["X"])
        capi.call("pdeip_pde_sor4_dev_to", st(), d["X"].data_ptr(), o.data_ptr(), *[d[k].data_ptr() for k in ("TRACE", "B", "wW", "wN", "wE", "wS")],
                  120, 96, 2, it, 1.75, 1, 0)
        assert pb.bit_equal(dev.to_matlab(o), oracle.pde_sor4(*f.values(), it, 1.75, oracle.COLOUR))


@pytest.mark.parametrize("small,pipe", [("1", "1"), ("0", "1"), ("0", "0")])
@pytest.mark.parametrize("shape", [(24, 40), (33, 29), (68, 120), (64, 96), (100, 48), (17, 30), (9, 15), (3, 3), (4, 5), (135, 240), (270, 100)])
def test_red_black_kernel_families_agree(pdeip, oracle, shape, small, pipe):
    """The three red-black kernel families -- one workgroup per small frame (k_sor_small), the four-sweep wave pipeline
    (k_sor_rbp) and the one/two-sweep marches (k_sor_rb) -- are selected by frame size; switched by hand they must all give
    the oracle's colour-ordered result on the same frames, every 5-point model, iter 1..9, NaN-laced data.

    The knobs only ALLOW a family: with the small path off and the pipeline on, a frame whose row count is not a multiple
    of 4 -- (33,29), (17,30), (9,15), (135,240), (270,100) -- and every single-field model below 2^21 pixels still runs
    k_sor_rb.  Which family a call ran is therefore asserted on its launch count, as the model of the launch logic in
    seam_model.py predicts it (iter = 9: one launch of k_sor_small, three of a cut small frame or of the pipeline,
    4 + 4 + 1, five of k_sor_rb)."""
    import os

    import torch

    import seam_model as sm

    api = pdeip.mex_api
    lib = pdeip.capi.load()
    cus = torch.cuda.get_device_properties(0).multi_processor_count

    def ran(model, it, nframes=1):
        family = sm.family_of(model, shape[0], shape[1], nframes, it, small=small == "1", pipe=pipe == "1", num_cus=cus)
        want = sm.sweep_launches(family, model, shape[0], shape[1], nframes, it, cus)
        got = lib.pdeip_last_launch_count()
        assert got == want, "%s %s it=%d small=%s pipe=%s: %d launches, %s makes %d" % (model, shape, it, small, pipe, got, family, want)

    old = {k: os.environ.get(k) for k in ("PDEIP_RB_SMALL", "PDEIP_RB_PIPE")}
    os.environ["PDEIP_RB_SMALL"], os.environ["PDEIP_RB_PIPE"] = small, pipe
    api.set_mode(1)
    try:
        f = np.float32
        for it in (1, 4, 9):
            p = pb.elin4(961, *shape, nan_frac=0.02)
            for g, w in zip(api.Oflow_sor_elin4_2d(*p.values(), f(it), f(1.9), f(1)), oracle.Oflow_sor_elin4_2d(*p.values(), it, 1.9, order=oracle.COLOUR)):
                assert pb.bit_equal(g, w), "elin4 %s it=%d small=%s pipe=%s: %s" % (shape, it, small, pipe, pb.describe_mismatch(g, w))
            ran("elin4", it)
            q = pb.llin4(962, *shape, nan_frac=0.02)
            for g, w in zip(api.Oflow_sor_llin4_2d(*q.values(), f(it), f(1.9), f(1)), oracle.Oflow_sor_llin4_2d(*q.values(), it, 1.9, order=oracle.COLOUR)):
                assert pb.bit_equal(g, w), "llin4 %s it=%d" % (shape, it)
            ran("llin4", it)
            d = pb.disp4(963, *shape, nan_frac=0.02)
            assert pb.bit_equal(api.Disp_sor_llin4_2d(*d.values(), f(it), f(1.9), f(1)), oracle.Disp_sor_llin4_2d(*d.values(), it, 1.9, order=oracle.COLOUR))
            ran("disp4", it)
            e = pb.pde4(964, *shape, nframes=3, nan_frac=0.02)
            assert pb.bit_equal(api.PDEsolver4(*e.values(), f(it), f(1.75), f(1)), oracle.PDEsolver4(*e.values(), it, 1.75, order=oracle.COLOUR))
            ran("pde4", it, 3)
            y = pb.dispsym4(965, *shape, nan_frac=0.02)
            for g, w in zip(api.Disp_sor_llin_sym4_2d(*y.values(), f(it), f(1.9), f(1)), oracle.Disp_sor_llin_sym4_2d(*y.values(), it, 1.9, order=oracle.COLOUR)):
                assert pb.bit_equal(g, w)
            ran("dispsym4", it)
    finally:
        api.set_mode(0)
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("qpref", ["1", "2", "4"])
@pytest.mark.parametrize("shape", [(68, 120), (135, 240), (270, 96), (45, 500), (31, 33), (200, 301)])
def test_small_frame_slabs_in_place(pdeip, oracle, shape, qpref):
    """k_sor_small cuts a frame into column slabs with a halo of two columns per sweep; relaxed IN PLACE the workgroups gate
    their stores on a load counter.  Device-pointer entry points, every 5-point model, iter 1 / 4 / 9 (9 = three launches of
    4+4+1 sweeps when the frame is cut), the slab width steered through PDEIP_SMALL_Q, vs the oracle's colour order."""
    import importlib
    import os

    dev, capi = importlib.import_module("pde-based-image-processing_amd.device"), pdeip.capi
    old = os.environ.get("PDEIP_SMALL_Q")
    os.environ["PDEIP_SMALL_Q"] = qpref
    try:
        for it in (1, 4, 9):
            p = pb.elin4(971, *shape, nan_frac=0.02)
            d = {k: dev.to_device(v) for k, v in p.items()}
            dev.oflow_sor_elin4(*[d[k] for k in ("U", "V", "M", "Cu", "Cv", "Du", "Dv", "wW", "wN", "wE", "wS")], it, 1.9, capi.MODE_RED_BLACK)
            want = oracle.oflow_sor_elin4(*p.values(), it, 1.9, oracle.COLOUR)
            assert pb.bit_equal(dev.to_matlab(d["U"]), want[0]), "elin4 %s it=%d q=%s: %s" % (shape, it, qpref, pb.describe_mismatch(dev.to_matlab(d["U"]), want[0]))
            assert pb.bit_equal(dev.to_matlab(d["V"]), want[1])
            q = pb.llin4(972, *shape, nan_frac=0.02)
            d = {k: dev.to_device(v) for k, v in q.items()}
            dev.oflow_sor_llin4(*[d[k] for k in ("U", "V", "dU", "dV", "M", "Cu", "Cv", "Du", "Dv", "wW", "wN", "wE", "wS")], it, 1.9, capi.MODE_RED_BLACK)
            want = oracle.oflow_sor_llin4(*q.values(), it, 1.9, oracle.COLOUR)
            assert pb.bit_equal(dev.to_matlab(d["dU"]), want[0]), "llin4 %s it=%d q=%s: %s" % (shape, it, qpref, pb.describe_mismatch(dev.to_matlab(d["dU"]), want[0]))
            assert pb.bit_equal(dev.to_matlab(d["dV"]), want[1])
            e = pb.disp4(973, *shape, nan_frac=0.02)
            d = {k: dev.to_device(v) for k, v in e.items()}
            dev.disp_sor_llin4(*[d[k] for k in ("U", "dU", "Cu", "Du", "wW", "wN", "wE", "wS")], it, 1.9, capi.MODE_RED_BLACK)
            assert pb.bit_equal(dev.to_matlab(d["dU"]), oracle.disp_sor_llin4(*e.values(), it, 1.9, oracle.COLOUR)), "disp4 %s it=%d" % (shape, it)
            f = pb.pde4(974, *shape, nframes=3, nan_frac=0.02)
            d = {k: dev.to_device(v) for k, v in f.items()}
            dev.pde_sor4(*[d[k] for k in ("X", "TRACE", "B", "wW", "wN", "wE", "wS")], it, 1.75, capi.MODE_RED_BLACK)
            assert pb.bit_equal(dev.to_matlab(d["X"]), oracle.pde_sor4(*f.values(), it, 1.75, oracle.COLOUR)), "pde4 %s it=%d" % (shape, it)
        assert capi.load().pdeip_persist_error() == 0, capi.last_error()
    finally:
        if old is None:
            os.environ.pop("PDEIP_SMALL_Q", None)
        else:
            os.environ["PDEIP_SMALL_Q"] = old
