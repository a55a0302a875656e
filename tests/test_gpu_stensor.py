"""GPU: structure-tensor anisotropic diffusion (csrc/pdeip_stensor.hip) stage by stage against the numpy restatement
(stensor_ref.py).  Each stage is fed the GPU's own input, so nothing accumulates.

  gaussian            bit for bit with the library's own taps: every tile edge of the 64-row / 64-column tiles, a radius beyond the
                      frame, 1 and 3 frames, NaN and +Inf pixels
  structure_tensor    bit for bit on the same shapes, gray and colour, with and without each smoothing
  st_weights(_padded) within one float32 ulp (only exp is not correctly rounded on both sides), zero on the frame, symmetric bit for bit
  one step            the GPU's padded weights handed to the reference's PDEsolver8: bit for bit, both solvers in both orderings
  pdeip_diffusion8    equal to the stage calls composed in Python (flow_level.Diffusion8Level), in and out of place; launch count;
                      graph replay; host-pointer call, drivers.Diffusion8 and the MEX stub; tau = 0 and iters = 0; the scene's orderings
"""
import ctypes
import importlib

import numpy as np
import pytest

import oracle_lib
import problems as pb
import stensor_ref as ref
from test_diffusion import build_diff_stub
from test_mex_stubs import call

pytestmark = pytest.mark.gpu
F32 = np.float32
T = 64  # GAUSS_T of csrc/pdeip_stensor.hpp: the tile edge of both passes


def _eq(got, want, what):
    assert pb.bit_equal(got, want), "%s: %s" % (what, pb.describe_mismatch(got, want))


def _drv():
    return importlib.import_module("pde-based-image-processing_amd.drivers")


def _dev():
    return importlib.import_module("pde-based-image-processing_amd.device")


def _fl():
    return importlib.import_module("pde-based-image-processing_amd.flow_level")


def _image(seed, shape):
    """0..255 content with structure at several scales: oblique waves, a step and noise."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(shape[0], dtype=np.float64), np.arange(shape[1], dtype=np.float64), indexing="ij")
    planes = []
    for c in range(shape[2] if len(shape) == 3 else 1):
        P = 120 + 70 * np.sin(0.5 * i + 0.3 * j + c) + 40 * (j > shape[1] / 2) + rng.normal(0, 12, shape[:2])
        planes.append(np.clip(P, 0, 255))
    I = np.stack(planes, axis=2) if len(shape) == 3 else planes[0]
    return np.asfortranarray(I.astype(F32))


def _ordered(a):
    """float32 bit patterns as integers that order like the values (-0 and +0 coincide)."""
    b = np.ascontiguousarray(a, F32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7fffffff), b)


def _within_one_ulp(got, want, what):
    d = np.abs(_ordered(got) - _ordered(want))
    assert d.max() <= 1, "%s: %d values beyond one ulp, worst %d ulps" % (what, int((d > 1).sum()), int(d.max()))
    return int((d == 1).sum())


# ---- gaussian ---------------------------------------------------------------------------------------------------------------

SHAPES = [(3, 3), (3, 17), (17, 3), (T - 1, 5), (T, 5), (T + 1, 5), (2 * T + 1, 5), (5, T - 1), (5, T), (5, T + 1), (5, 2 * T + 1), (130, 66)]
SIGMAS = [0.0, 0.5, 1.25, 4.0, 10.6]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gaussian_bit_for_bit(pdeip, shape):
    dev = _dev()
    for F in (1, 3):
        I = _image(sum(shape) + F, shape + (F,) if F > 1 else shape)
        t = dev.to_device(I)
        for sigma in SIGMAS:
            g, R = dev.gauss_taps(sigma)
            got = dev.to_matlab(dev.gaussian(t, sigma))
            _eq(got, ref.gaussian(I, sigma, g), "%s x %d, sigma %g (R %d)" % (shape, F, sigma, R))
        _eq(dev.to_matlab(t), I, "the input after the calls")


def test_gaussian_host_pointer_call_and_refused_alias(pdeip):
    dev, drv = _dev(), _drv()
    I = _image(5, (70, 67, 3))
    g, _ = dev.gauss_taps(1.25)
    _eq(drv.gaussian(I, 1.25), ref.gaussian(I, 1.25, g), "drivers.gaussian")
    _eq(drv.gaussian(I[:, :, 0], 0), I[:, :, 0], "sigma = 0")
    t = dev.to_device(I)
    with pytest.raises(pdeip.PdeipError, match="aliases"):
        dev.gaussian(t, 1.0, out=t)


@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
def test_gaussian_non_finite_pixels(pdeip, value):
    dev = _dev()
    for where in ((9, 40), (0, 0), (19, 69)):
        I = _image(11, (20, 70))
        I[where] = value
        for sigma in (0.5, 4.0):
            g, _ = dev.gauss_taps(sigma)
            got, want = dev.to_matlab(dev.gaussian(dev.to_device(I), sigma)), ref.gaussian(I, sigma, g)
            assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want)), (where, sigma)
            ok = np.isfinite(want)
            assert ok.any() and not ok.all()
            assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32)), (where, sigma)


# ---- structure tensor -------------------------------------------------------------------------------------------------------

def _gpu_tensor(dev, I, sigma, rho):
    import torch

    t = dev.to_device(I)
    planes = t if t.dim() == 3 else t[None]
    J = torch.empty((3,) + tuple(planes.shape[-2:]), dtype=torch.float32, device=t.device)
    dev.structure_tensor(planes, sigma, rho, J)
    return J


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_structure_tensor_bit_for_bit(pdeip, shape):
    dev = _dev()
    for C in (1, 3):
        I = _image(3 * sum(shape) + C, shape + (C,) if C > 1 else shape)
        for sigma, rho in ((0.0, 0.0), (0.7, 0.0), (0.7, 4.0), (1.5, 1.25)):
            gs, gr = dev.gauss_taps(sigma)[0], dev.gauss_taps(rho)[0]
            got = dev.to_matlab(_gpu_tensor(dev, I, sigma, rho))
            _eq(got, ref.structure_tensor(I, sigma, rho, gs, gr), "%s x %d, sigma %g, rho %g" % (shape, C, sigma, rho))


# ---- weights ----------------------------------------------------------------------------------------------------------------

def _stripes(sign, shape=(40, 70)):
    y, x = np.meshgrid(np.arange(shape[0], dtype=np.float64), np.arange(shape[1], dtype=np.float64), indexing="ij")
    return np.asfortranarray((128.0 + 100.0 * np.sin(0.8 * (x - sign * y))).astype(F32))


WEIGHT_IMAGES = {"textured": lambda: _image(21, (66, 130, 3)), "flat": lambda: np.full((9, 70), 80.0, F32, order="F"),
                 "stripes+": lambda: _stripes(1), "stripes-": lambda: _stripes(-1), "3x3": lambda: _image(22, (3, 3))}


@pytest.mark.parametrize("mode", ["ced", "eed"])
@pytest.mark.parametrize("image", list(WEIGHT_IMAGES))
def test_weights(pdeip, image, mode):
    import torch

    dev = _dev()
    I = WEIGHT_IMAGES[image]()
    p = ref.params(mode)
    prm = dev.diffusion8_params(mode)
    J = _gpu_tensor(dev, I, p["sigma"], p["rho"])
    nc, nr = J.shape[-2:]
    for tau in (1.0, 0.37):
        TRACE, w8 = torch.empty((nc, nr), dtype=torch.float32, device=J.device), torch.empty((8, nc, nr), dtype=torch.float32, device=J.device)
        dev.st_weights(J, prm, tau, TRACE, w8)
        gT, gw = dev.to_matlab(TRACE), dev.to_matlab(w8)
        wT, ww = ref.st_weights(dev.to_matlab(J), mode, p, tau)
        off = _within_one_ulp(gT, wT, "TRACE")
        for k in range(8):
            off += _within_one_ulp(gw[:, :, k], ww[k], "weight %d" % k)
        print("%s %s tau %g: %d of %d values one ulp off" % (image, mode, tau, off, 9 * gT.size))
        # zero in exactly the frame positions TVdenoise8's assembly zeroes
        frame = [np.zeros((nr, nc), bool) for _ in range(8)]
        for k in (0, 1, 7):
            frame[k][:, 0] = True
        for k in (3, 4, 5):
            frame[k][:, -1] = True
        for k in (1, 2, 3):
            frame[k][0, :] = True
        for k in (5, 6, 7):
            frame[k][-1, :] = True
        for k in range(8):
            assert not gw[:, :, k][frame[k]].any(), "weight %d is not zero on the frame" % k
            assert np.array_equal(gw[:, :, k] == 0, ww[k] == 0), "weight %d: zeros elsewhere differ" % k
        W, NW, N, NE, E, SE, S, SW = (gw[:, :, k] for k in range(8))
        bits = lambda a: np.ascontiguousarray(a).view(np.uint32)  # noqa: E731
        assert np.array_equal(bits(E[:, :-1]), bits(W[:, 1:])) and np.array_equal(bits(S[:-1]), bits(N[1:]))
        assert np.array_equal(bits(SE[:-1, :-1]), bits(NW[1:, 1:])) and np.array_equal(bits(NE[1:, :-1]), bits(SW[:-1, 1:]))
        # the padded form: the same values inside a ring of TRACE = 1 and zero weights
        TRp = torch.full((nc + 2, nr + 2), 7.0, dtype=torch.float32, device=J.device)
        w8p = torch.full((8, nc + 2, nr + 2), 7.0, dtype=torch.float32, device=J.device)
        dev.st_weights_padded(J, prm, tau, TRp, w8p)
        wantT, wantw = ref.pad_weights(gT, [gw[:, :, k] for k in range(8)])
        _eq(dev.to_matlab(TRp), wantT, "padded TRACE")
        for k in range(8):
            _eq(dev.to_matlab(w8p)[:, :, k], wantw[k], "padded weight %d" % k)
    if image == "flat":
        assert np.abs(gT[1:-1, 1:-1] - (1 + 0.37 * 4 * (0.001 if mode == "ced" else 1.0))).max() <= 2.0 ** -22  # the isotropic 5-point row
    if image.startswith("stripes") and mode == "ced":
        sign = 1 if image.endswith("+") else -1
        mid = gw[12:-12, 12:-12, 1] / F32(0.37)   # wNW = (D12 + D12') / 4: +-(1 - alpha) / 4
        assert np.abs(mid - sign * 0.24975).max() <= 1e-3


def test_pad_and_crop(pdeip):
    import torch

    dev = _dev()
    for shape in ((3, 3), (5, 2 * T + 1, 3), (257, 4)):
        I = _image(31, shape)
        t = dev.to_device(I)
        want = np.pad(I, ((1, 1), (1, 1)) + ((0, 0),) * (I.ndim - 2), mode="edge")
        a = torch.zeros(tuple(t.shape[:-2]) + (t.shape[-2] + 2, t.shape[-1] + 2), dtype=torch.float32, device=t.device)
        b = torch.zeros_like(a)
        dev.st_pad(t, a, b)
        _eq(dev.to_matlab(a), want, "pad %s" % (shape,))
        _eq(dev.to_matlab(b), want, "pad, second output")
        back = torch.zeros_like(t)
        dev.st_crop(a, back)
        _eq(dev.to_matlab(back), I, "crop %s" % (shape,))


# ---- one step ---------------------------------------------------------------------------------------------------------------

STEP_CASES = [(1, 0), (1, 1), (2, 0), (2, 1)]   # (solver, library mode = oracle order)


@pytest.mark.parametrize("solver,order", STEP_CASES, ids=["sor-exact", "sor-colour", "alr-exact", "alr-zebra"])
@pytest.mark.parametrize("shape", [(3, 3), (17, 33), (66, 130, 3)], ids=lambda s: "x".join(map(str, s)))
def test_one_step_equals_the_reference_solver(pdeip, shape, solver, order):
    import torch

    dev = _dev()
    I = _image(41, shape)
    for mode in ("ced", "eed"):
        p = ref.params(mode, solver=solver)
        prm = dev.diffusion8_params(mode)
        t = dev.to_device(I)
        planes = t if t.dim() == 3 else t[None]
        C, nc, nr = planes.shape
        J = _gpu_tensor(dev, I, p["sigma"], p["rho"])
        TRp = torch.empty((nc + 2, nr + 2), dtype=torch.float32, device=t.device)
        w8p = torch.empty((8, nc + 2, nr + 2), dtype=torch.float32, device=t.device)
        X, B = torch.empty((C, nc + 2, nr + 2), dtype=torch.float32, device=t.device), torch.empty((C, nc + 2, nr + 2), dtype=torch.float32, device=t.device)
        dev.st_weights_padded(J, prm, p["tau"], TRp, w8p)
        dev.st_pad(planes, X, B)
        hT, hw, hX = dev.to_matlab(TRp), dev.to_matlab(w8p), dev.to_matlab(X)
        solve = dev.pde_sor8 if solver == 1 else dev.pde_alr8
        for c in range(C):
            solve(X[c], TRp, B[c], *w8p, p["inner_iter"], p["omega"], order)
        dev.sync_check()
        got = dev.to_matlab(X)
        for c in range(C):
            want = ref.step_padded(np.asfortranarray(hX[:, :, c]), hT, [np.asfortranarray(hw[:, :, k]) for k in range(8)], p, order)
            _eq(got[:, :, c], want, "%s %s channel %d" % (mode, shape, c))
            assert not pb.bit_equal(want, hX[:, :, c])


# ---- the driver -------------------------------------------------------------------------------------------------------------

def _launches(pdeip):
    return pdeip.capi.load().pdeip_last_launch_count()


def _solver_launches(pdeip, dev, nrows, ncols, p, order):
    """What the solver call on one ringed plane reports."""
    import torch

    X, TRACE, B = (torch.ones((ncols + 2, nrows + 2), dtype=torch.float32, device="cuda") for _ in range(3))
    w8 = torch.zeros((8, ncols + 2, nrows + 2), dtype=torch.float32, device="cuda")   # consecutive planes, as the driver has them
    (dev.pde_sor8 if p["solver"] == 1 else dev.pde_alr8)(X, TRACE, B, *w8, p["inner_iter"], p["omega"], order)
    return _launches(pdeip)


@pytest.mark.parametrize("mode,solver,order", [("ced", 1, 0), ("eed", 1, 0), ("ced", 2, 0), ("eed", 2, 1), ("ced", 1, 1)])
def test_driver_equals_the_composed_stages(pdeip, mode, solver, order):
    import torch

    dev, fl = _dev(), _fl()
    old = pdeip.capi.get_mode()
    pdeip.capi.set_mode(order)
    try:
        for shape in ((17, 33), (66, 130, 3)):
            I = _image(51, shape)
            p = ref.params(mode, solver=solver, iters=3)
            prm = dev.diffusion8_params(mode, solver=solver, iters=3)
            t = dev.to_device(I)
            want = dev.to_matlab(fl.Diffusion8Level(mode, p, order).run(t))
            _eq(dev.to_matlab(t), I, "Iin after the composed run")
            out = torch.zeros_like(t)
            dev.diffusion8(t, prm, out)
            count = _launches(pdeip)
            _eq(dev.to_matlab(out), want, "out of place %s" % (shape,))
            _eq(dev.to_matlab(t), I, "Iin after an out-of-place call")
            C = shape[2] if len(shape) == 3 else 1
            L = _solver_launches(pdeip, dev, shape[0], shape[1], p, order)
            S = 2 * (p["sigma"] > 0) + 1 + 2 * (p["rho"] > 0)
            assert count == 1 + 3 * (S + 3 + C * L), (count, S, L)
            dev.diffusion8(t, prm, t)
            assert _launches(pdeip) == count - 1
            _eq(dev.to_matlab(t), want, "in place %s" % (shape,))
            assert not pb.bit_equal(want, I)
        dev.sync_check()
    finally:
        pdeip.capi.set_mode(old)


def test_driver_eager_and_graph_replayed(pdeip):
    """Captured on a side stream after an eager call has created the workspaces.  Red-black point SOR, the solver the drivers' graph
    replay already runs."""
    import torch

    dev = _dev()
    I = _image(61, (66, 130, 3))
    prm = dev.diffusion8_params("ced", iters=3)
    old = pdeip.capi.get_mode()
    pdeip.capi.set_mode(1)
    try:
        t = dev.to_device(I)
        out = torch.empty_like(t)
        dev.diffusion8(t, prm, out)
        torch.cuda.synchronize()
        eager = dev.to_matlab(out)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            dev.diffusion8(t, prm, out)
        torch.cuda.current_stream().wait_stream(side)
        for _ in range(3):
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            _eq(dev.to_matlab(out), eager, "graph replay")
        _eq(dev.to_matlab(t), I, "I after the replays")
    finally:
        pdeip.capi.set_mode(old)
    dev.sync_check()


def test_every_entry_gives_the_device_result(pdeip):
    import torch

    dev, drv = _dev(), _drv()
    I = _image(71, (40, 53, 3))
    lib = build_diff_stub("Diffusion8_gpu", pdeip)
    for mode, kw in (("ced", {}), ("eed", {"lambda": 4.0, "iters": 2, "solver": 2})):
        t = dev.to_device(I)
        out = torch.empty_like(t)
        dev.diffusion8(t, dev.diffusion8_params(mode, **kw), out)
        want = dev.to_matlab(out)
        _eq(drv.capi_Diffusion8(I, mode, as_single=True, **kw), want, "host-pointer call %s" % mode)
        _eq(drv.Diffusion8(I, mode, as_single=True, **kw), want, "drivers.Diffusion8 %s" % mode)
        got8 = drv.Diffusion8(I, mode, **kw)
        assert got8.dtype == np.uint8 and np.array_equal(got8, drv.uint8_matlab(want))
        nan = np.nan
        pv = np.array([0.0 if mode == "eed" else 1.0, nan, nan, kw.get("lambda", nan), nan, nan, nan, kw.get("iters", nan), nan, nan, kw.get("solver", nan)])
        err, outs = call(lib, 1, [I, pv])
        assert err is None, err
        _eq(outs[0], want, "MEX stub %s" % mode)
    err, _ = call(lib, 1, [I, np.zeros(10)])
    assert err == "Diffusion8_gpu: 'params' must be a real double vector of 11 elements"
    gray = drv.Diffusion8(I[:, :, 0], as_single=True)
    assert gray.shape == I.shape[:2]


def test_tau_zero_and_no_iterations_return_the_input(pdeip):
    drv = _drv()
    I = _image(81, (17, 33, 3))
    for fn in (drv.Diffusion8, drv.capi_Diffusion8):
        for mode in ("ced", "eed"):
            _eq(fn(I, mode, as_single=True, tau=0), I, "tau = 0")
            _eq(fn(I, mode, as_single=True, iters=0), I, "iters = 0")
            _eq(fn(I, mode, as_single=True, iters=-3), I, "iters < 0")


def test_scene_orderings_on_the_gpu(pdeip):
    drv = _drv()
    clean, noisy = ref.stripe_scene()
    noisy32 = np.asfortranarray(noisy.astype(F32))
    fig = {"gauss%g" % s: ref.rms(drv.gaussian(noisy32, s), clean) for s in (1.0, 1.5, 2.0)}
    fig["diffusion4"] = ref.rms(drv.Diffusion4_v10(noisy32, as_single=True), clean)
    fig["eed"] = ref.rms(drv.Diffusion8(noisy32, "eed", as_single=True), clean)
    fig["ced"] = ref.rms(drv.Diffusion8(noisy32, "ced", as_single=True), clean)
    print("RMS against the clean image on the GPU: " + ", ".join("%s %.2f" % kv for kv in fig.items()))
    best = min(fig["gauss1"], fig["gauss1.5"], fig["gauss2"])
    assert fig["ced"] < best and fig["ced"] < fig["diffusion4"]
    assert fig["eed"] < best
    # the restatement's figures, to the effect of the one-ulp differences in the weights
    assert abs(fig["ced"] - ref.rms(ref.Diffusion8(noisy32, "ced"), clean)) <= 0.01
    assert abs(fig["eed"] - ref.rms(ref.Diffusion8(noisy32, "eed"), clean)) <= 0.01
