"""CPU: the numpy restatement of structure-tensor anisotropic diffusion (stensor_ref.py) on its own, and pdeip_gauss_taps, the one
host-only entry point, against it.

The restatement is what tests/test_gpu_stensor.py compares the GPU with bit for bit.  Here it is pinned to what does not depend
on it: a direct float64 convolution, the closed forms of the 9-point stencil under a constant tensor, the symmetry and the row
sums the semi-implicit system needs, the orientation of the tensor, and the quality of the filter on a scene with ground truth."""
import ctypes
import functools
import importlib
import math

import numpy as np
import pytest

import diffusion_ref
import stensor_ref as ref

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _ulps(a, b):
    """Distance in float32 units in the last place (same-sign finite values)."""
    ia, ib = _bits(a).astype(np.int64), _bits(b).astype(np.int64)
    return np.abs(ia - ib)


def _image(seed, shape):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(rng.uniform(0, 255, shape).astype(F32))


# ---- the Gaussian -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sigma", [0.5, 1.25, 4.0])
def test_separable_gaussian_equals_the_direct_convolution(sigma):
    """Each of the two passes adds 2R + 1 products of magnitude <= 255 g[k] in float32: the error of a pass is below
    (2R + 2) x 2^-24 x 255 (the taps sum to 1), the tap rounding adds 2^-24 x 255 per pass, and the second pass carries the first's
    error through weights that sum to 1: 2 (2R + 3) 2^-24 x 255 in all."""
    I = _image(3, (23, 31))
    R = ref.radius(sigma)
    got = ref.gaussian(I, sigma)
    assert got.dtype == F32
    err = np.abs(got.astype(np.float64) - ref.gaussian_direct64(I, sigma)).max()
    bound = 2 * (2 * R + 3) * 2.0 ** -24 * 255
    print("sigma %g: R %d, max error %.3g, bound %.3g" % (sigma, R, err, bound))
    assert err <= bound
    assert err > 0 or sigma == 0


def test_sigma_zero_is_a_copy_and_the_border_replicates():
    I = _image(4, (5, 7))
    assert np.array_equal(_bits(ref.gaussian(I, 0.0)), _bits(I))
    flat = np.full((4, 6), 37.25, F32)
    assert np.abs(ref.gaussian(flat, 4.0) - 37.25).max() <= 37.25 * 30 * 2.0 ** -24  # radius 12 > the frame: all replicate


TAPS = [(0.0, 0), (0.3, 1), (0.5, 2), (1.25, 4), (4.0, 12), (10.6, 32)]


@pytest.mark.parametrize("sigma,R", TAPS)
def test_library_taps_equal_the_restatement(pdeip, sigma, R):
    dev = importlib.import_module("pde-based-image-processing_amd.device")
    g, r = dev.gauss_taps(sigma)
    want = ref.taps(sigma)
    assert r == R == ref.radius(sigma) and len(g) == 2 * R + 1 == len(want)
    assert _ulps(g, want).max() <= 1, (g, want)
    assert abs(float(g.astype(np.float64).sum()) - 1.0) <= (2 * R + 1) * 2.0 ** -25
    assert np.array_equal(g, g[::-1])


def test_library_taps_refusals(pdeip):
    capi = pdeip.capi
    buf = (ctypes.c_float * 65)(*([7.0] * 65))
    R = ctypes.c_int(-5)
    a = ctypes.addressof(buf)
    for sigma, code, msg in ((10.7, capi.PDEIP_ERR_UNSUPPORTED, "radius"), (math.nan, capi.PDEIP_ERR_ARG, "sigma"), (-0.5, capi.PDEIP_ERR_ARG, "sigma"),
                             (math.inf, capi.PDEIP_ERR_ARG, "sigma")):
        with pytest.raises(capi.PdeipError) as e:
            capi.call("pdeip_gauss_taps", sigma, a, 65, ctypes.byref(R))
        assert e.value.code == code and msg in str(e.value) and "pdeip_gauss_taps" in str(e.value)
    with pytest.raises(capi.PdeipError, match="capacity"):
        capi.call("pdeip_gauss_taps", 1.25, a, 8, ctypes.byref(R))
    with pytest.raises(capi.PdeipError, match="NULL"):
        capi.call("pdeip_gauss_taps", 1.25, None, 65, ctypes.byref(R))
    assert list(buf) == [7.0] * 65 and R.value == -5
    with pytest.raises(ValueError):
        ref.taps(10.7)


# ---- the stencil ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D11,D22,D12", [(1.0, 1.0, 0.0), (0.7, 0.2, 0.3), (0.05, 0.9, -0.2)])
def test_stencil_is_consistent_under_a_constant_tensor(D11, D22, D12):
    """With dyy := D11, dxx := D22, dxy := D12 the eight weights applied to x y, x^2, y^2 give 2 D12, 2 D11, 2 D22 in the interior."""
    shape = (9, 11)
    y, x = np.meshgrid(np.arange(shape[0], dtype=np.float64), np.arange(shape[1], dtype=np.float64), indexing="ij")
    w, total = ref.weights64(np.full(shape, D11), np.full(shape, D22), np.full(shape, D12))
    for u, want in ((x * y, 2 * D12), (x * x, 2 * D11), (y * y, 2 * D22), (x, 0.0), (y, 0.0)):
        got = ref.apply_stencil(u, w)[1:-1, 1:-1]
        assert np.abs(got - want).max() <= 1e-13, (want, got)
    assert np.abs(total[1:-1, 1:-1] - (2 * D11 + 2 * D22)).max() <= 1e-15  # the diagonal weights cancel in the sum


def _scene_weights(mode):
    _, noisy = ref.stripe_scene()
    p = ref.params(mode)
    J = ref.structure_tensor(noisy.astype(F32), p["sigma"], p["rho"])
    return ref.st_weights(J, mode, p, 1.0)


@pytest.mark.parametrize("mode", ["ced", "eed"])
def test_weights_are_symmetric_bit_for_bit(mode):
    _, (W, NW, N, NE, E, SE, S, SW) = _scene_weights(mode)
    assert np.array_equal(_bits(E[:, :-1]), _bits(W[:, 1:]))
    assert np.array_equal(_bits(S[:-1]), _bits(N[1:]))
    assert np.array_equal(_bits(SE[:-1, :-1]), _bits(NW[1:, 1:]))
    assert np.array_equal(_bits(NE[1:, :-1]), _bits(SW[:-1, 1:]))
    assert NW.any() and NE.any()  # the tensor is not diagonal on this scene


@pytest.mark.parametrize("mode", ["ced", "eed"])
def test_frame_weights_are_zero(mode):
    _, w = _scene_weights(mode)
    for k in (0, 1, 7):
        assert not w[k][:, 0].any()
    for k in (3, 4, 5):
        assert not w[k][:, -1].any()
    for k in (1, 2, 3):
        assert not w[k][0, :].any()
    for k in (5, 6, 7):
        assert not w[k][-1, :].any()
    assert w[0][1:-1, 1:].all() and w[2][1:, 1:-1].all()


@pytest.mark.parametrize("tau", [1.0, 0.37])
@pytest.mark.parametrize("mode", ["ced", "eed"])
def test_row_sums(mode, tau):
    """TRACE - sum w8 == 1: TRACE and the eight weights are each rounded once from float64 (relative 2^-24 of values <= 1 + 4 tau),
    and the float64 sum of nine such values is exact to 2^-50."""
    _, noisy = ref.stripe_scene()
    p = ref.params(mode)
    J = ref.structure_tensor(noisy.astype(F32), p["sigma"], p["rho"])
    TRACE, w8 = ref.st_weights(J, mode, p, tau)
    s = TRACE.astype(np.float64) - sum(v.astype(np.float64) for v in w8)
    assert np.abs(s - 1.0).max() <= 9 * (1 + 4 * tau) * 2.0 ** -24


def _stripes(sign):
    y, x = np.meshgrid(np.arange(40.0), np.arange(48.0), indexing="ij")
    return (128.0 + 100.0 * np.sin(0.8 * (x - sign * y))).astype(F32)   # constant along (1, sign)


@pytest.mark.parametrize("sign", [1, -1])
def test_orientation(sign):
    """Stripes running along (1, 1) (x along the columns, y down the rows) make CED smooth along (1, 1): D12 = +(1 - alpha) / 2;
    along (1, -1): the same with a minus."""
    p = ref.params("ced")
    J = ref.structure_tensor(_stripes(sign), p["sigma"], p["rho"])
    D11, D22, D12 = ref.diffusion_tensor(J, "ced", p)
    mid = D12[12:-12, 12:-12]
    print("D12 in the interior: %.4f .. %.4f" % (mid.min(), mid.max()))
    assert np.abs(mid - sign * 0.4995).max() <= 1e-3
    assert np.abs(D11[12:-12, 12:-12] - 0.5005).max() <= 1e-3 and np.abs(D22[12:-12, 12:-12] - 0.5005).max() <= 1e-3
    # EED on the same image: diffusion across the stripes (the gradient direction (1, -sign)) is shut off
    pe = ref.params("eed")
    E11, E22, E12 = ref.diffusion_tensor(ref.structure_tensor(_stripes(sign), pe["sigma"], pe["rho"]), "eed", pe)
    across = 0.5 * (E11 + E22) - sign * E12   # v' D v for v = (1, -sign) / sqrt 2
    along = 0.5 * (E11 + E22) + sign * E12
    assert np.median(across) < 0.05 and np.median(along) > 0.95


def test_flat_image_gives_the_isotropic_tensor():
    flat = np.full((7, 9), 80.0, F32)
    for mode, diag in (("ced", 0.001), ("eed", 1.0)):
        p = ref.params(mode)
        J = ref.structure_tensor(flat, p["sigma"], p["rho"])
        assert not J.any()
        D11, D22, D12 = ref.diffusion_tensor(J, mode, p)
        assert np.all(D11 == diag) and np.all(D22 == diag) and not D12.any()


# ---- the filter on the scene ----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def scene_figures():
    """RMS against the clean stripes of: the noisy input, three Gaussians, Diffusion4_v10, EED and CED at their defaults."""
    clean, noisy = ref.stripe_scene()
    noisy32 = np.asfortranarray(noisy.astype(F32))
    fig = {"noisy": ref.rms(noisy32, clean)}
    for s in (1.0, 1.5, 2.0):
        fig["gauss%g" % s] = ref.rms(ref.gaussian(noisy32, s), clean)
    fig["diffusion4"] = ref.rms(diffusion_ref.Diffusion4_v10(noisy32), clean)
    fig["eed"] = ref.rms(ref.Diffusion8(noisy32, "eed"), clean)
    fig["ced"] = ref.rms(ref.Diffusion8(noisy32, "ced"), clean)
    return fig


def test_scene_orderings():
    fig = scene_figures()
    print("RMS against the clean image: " + ", ".join("%s %.2f" % kv for kv in fig.items()))
    best_gauss = min(fig["gauss1"], fig["gauss1.5"], fig["gauss2"])
    assert fig["ced"] < best_gauss and fig["ced"] < fig["diffusion4"]
    assert fig["eed"] < best_gauss
    assert best_gauss < fig["noisy"]


def test_mean_is_preserved_by_the_exact_solve():
    """The system matrix is symmetric with unit row sums, so an exact solve keeps the image mean: assemble it densely on a small
    crop in float64 and solve."""
    _, noisy = ref.stripe_scene()
    I = noisy[:14, :18]
    p = ref.params("ced")
    J = ref.structure_tensor(I.astype(F32), p["sigma"], p["rho"])
    w, total = ref.weights64(*ref.diffusion_tensor(J, "ced", p))
    nr, nc = I.shape
    n = nr * nc
    A = np.zeros((n, n))
    off = [(0, -1), (-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1)]
    for i in range(nr):
        for j in range(nc):
            q = i * nc + j
            A[q, q] = 1.0 + total[i, j]
            for k, (di, dj) in enumerate(off):
                if w[k][i, j] != 0.0:
                    A[q, (i + di) * nc + (j + dj)] -= w[k][i, j]
    assert np.abs(A - A.T).max() == 0.0
    x = np.linalg.solve(A, I.ravel())
    assert abs(x.mean() - I.mean()) <= 1e-11 * abs(I.mean())
    assert np.abs(x - I.ravel()).max() > 1.0  # the step did something
