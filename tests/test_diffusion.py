"""CPU: Diffusion4_v10 (matlab/diffusion/Diffusion4_v10.m) at the boundary, and its numpy restatement (diffusion_ref.py) on
its own.

The restatement is what tests/test_gpu_diffusion.py compares the GPU with bit for bit.  Here its weight half is pinned to the
reference's own compiled DdiffWeights gateway (oracle/_ref/, eps = single(1e-5), frame 0), its solver half to a scalar
transcription of TDMA (:70-92), and its algebra to the conservation the systems imply."""
import ctypes
import importlib
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import diffusion_ref as ref
import problems as pb
import ref_lib
from test_capi_symbols import declared_symbols
from test_mex_stubs import MOCK_DIR, ROOT, call

F32 = np.float32
ENTRIES = ["pdeip_diffusion4", "pdeip_diffusion4_dev"]
DIFF_DIR = os.path.join(ROOT, "pde-based-image-processing_amd", "mex", "diffusion")
BUILD_DIR = os.path.join(MOCK_DIR, "_build")


def drivsco():
    """single(I) of the two drivsco images [320, 400, 3], 0..255 as the driver takes them."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "levelset", "drivsco.npz"))
    return [np.asfortranarray(z[k].astype(F32)) for k in ("I1", "I2")]


def gray(seed=7, shape=(37, 53)):
    """A gray synthetic image: a smooth ramp, a bright square and noise, 0..255."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    I = 2.0 * i + 1.5 * j + rng.normal(0, 8, shape)
    I[shape[0] // 4:shape[0] // 2, shape[1] // 3:2 * shape[1] // 3] += 90
    return np.asfortranarray(np.clip(I, 0, 255).astype(F32))


def build_diff_stub(name, pdeip):
    """Compile mex/diffusion/<name>.c against the mock MEX runtime (tests/mexmock) and libpdeip.so."""
    os.makedirs(BUILD_DIR, exist_ok=True)
    so = os.path.join(BUILD_DIR, "diffusion_" + name + ".so")
    srcs = [os.path.join(DIFF_DIR, name + ".c"), os.path.join(MOCK_DIR, "mexmock.c")]
    deps = srcs + [os.path.join(DIFF_DIR, "..", "pdeip_mex_util.h"), os.path.join(MOCK_DIR, "mex.h"), pdeip.capi.LIB_PATH]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        libdir = os.path.dirname(pdeip.capi.LIB_PATH)
        subprocess.run(["gcc", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-shared", "-fPIC", "-I" + MOCK_DIR,
                        "-I" + os.path.join(ROOT, "include"), "-o", so] + srcs + ["-L" + libdir, "-lpdeip", "-Wl,-rpath," + libdir],
                       check=True)
    lib = ctypes.CDLL(so)
    lib.mock_make.restype = ctypes.c_void_p
    lib.mock_make.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_long), ctypes.c_int, ctypes.c_void_p]
    lib.mock_free.argtypes = [ctypes.c_void_p]
    lib.mock_data.restype = ctypes.c_void_p
    lib.mock_data.argtypes = [ctypes.c_void_p]
    lib.mock_ndim.argtypes = [ctypes.c_void_p]
    lib.mock_dim.restype = ctypes.c_long
    lib.mock_dim.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.mock_last_error.restype = ctypes.c_char_p
    lib.mock_call.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    return lib


def _eq(got, want, what):
    assert pb.bit_equal(got, want), "%s: %s" % (what, pb.describe_mismatch(got, want))


# ---- the weights against the reference's own DdiffWeights ---------------------------------------------------------------------

def _require_ref_build():
    """As tests/test_ref_oracle.py: with a reference checkout at hand a missing or stale oracle/_ref/ is a failure; only when
    neither the checkout nor a build exists is the comparison skipped."""
    spec = importlib.util.spec_from_file_location("pdeip_build_ref", os.path.join(ROOT, "oracle", "build_ref.py"))
    br = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(br)
    tree = br.reference_dir()
    if tree is not None:
        if not br.up_to_date(tree):
            pytest.fail("oracle/_ref/ is missing or stale against the reference at %s: run `python __graft_entry__.py build`" % tree)
    elif ref_lib.available() is None:
        pytest.skip("no reference checkout and no oracle/_ref/ build: nothing to compare the weights with")
    assert ref_lib.available() is not None, "oracle/_ref/MANIFEST.json does not describe this tree's stand-in runtime"


@pytest.mark.parametrize("image", ["drivsco1", "drivsco2", "gray"])
def test_weights_equal_the_reference_gateway(image):
    _require_ref_build()
    D = {"drivsco1": lambda: drivsco()[0], "drivsco2": lambda: drivsco()[1], "gray": gray}[image]()
    got = ref_lib.call("DdiffWeights", 4, D, F32(1e-5))
    want = ref.diff_weights(D)
    for name, g, w in zip(("wW", "wN", "wE", "wS"), got, want):
        g3 = g if g.ndim == 3 else g[:, :, None]
        _eq(g3[:, :, 0], w, "%s %s" % (image, name))
        assert not g3[:, :, 1:].any(), "%s: the gateway wrote frames above 0" % name


def test_weights_are_symmetric():
    """wS(i) and wN(i+1) are the same sum of the same squares, as are wE(j) and wW(j+1): the systems are symmetric."""
    wW, wN, wE, wS = ref.diff_weights(drivsco()[0])
    assert np.array_equal(wS[:-1].view(np.uint32), wN[1:].view(np.uint32))
    assert np.array_equal(wE[:, :-1].view(np.uint32), wW[:, 1:].view(np.uint32))


# ---- the solver against a scalar transcription of TDMA ------------------------------------------------------------------------

def _tdma_scalar(a, b, c, d):
    """Diffusion4_v10.m:70-92 on one column, one float32 scalar operation at a time."""
    n = len(a)
    c, d = [F32(v) for v in c], [F32(v) for v in d]
    c[0] = c[0] / b[0]
    d[0] = d[0] / b[0]
    for i in range(1, n - 1):
        temp = F32(1) / (b[i] - a[i] * c[i - 1])
        c[i] = c[i] * temp
        d[i] = (d[i] - a[i] * d[i - 1]) * temp
    d[n - 1] = (d[n - 1] - a[n - 1] * d[n - 2]) / (b[n - 1] - a[n - 1] * c[n - 2])
    x = [F32(0)] * n
    x[n - 1] = d[n - 1]
    for i in range(n - 2, -1, -1):
        x[i] = d[i] - c[i] * x[i + 1]
    return np.array(x, F32)


@pytest.mark.parametrize("n", [2, 3, 9, 300])
def test_vectorised_tdma_equals_the_scalar_transcription(n):
    rng = np.random.default_rng(n)
    m = 6
    a = (-rng.uniform(0, 40, (n, m))).astype(F32)
    c = (-rng.uniform(0, 40, (n, m))).astype(F32)
    b = (F32(2) - a - c + rng.uniform(0, 1, (n, m)).astype(F32)).astype(F32)  # diagonally dominant
    d = rng.uniform(0, 255, (n, m)).astype(F32)
    got = ref.tdma(a, b, c, d)
    assert got.dtype == F32
    for j in range(m):
        want = _tdma_scalar(list(a[:, j]), list(b[:, j]), list(c[:, j]), list(d[:, j]))
        _eq(got[:, j], want, "column %d of n = %d" % (j, n))


def test_tdma_refuses_lines_shorter_than_two():
    with pytest.raises(ValueError):
        ref.tdma(*[np.ones((1, 3), F32)] * 4)


# ---- the algebra: each iteration keeps every channel's sum ---------------------------------------------------------------------

def test_iterations_preserve_each_channel_sum_in_float64():
    """wS(i) = wN(i+1) and a + b + c = 2 make every system symmetric with row sums 2, so its solution sums to sum(d)/2 in exact
    arithmetic, and ver + hor keeps each channel's sum.  The rounding bound (line length x condition ~ 400 x 1.6e4 x 2^-53 ~ 7e-10)
    is below the 1e-9 asked; a coefficient in the wrong place (a and c swapped) breaks the sum by far more."""
    I = ref.Diffusion4_v10(drivsco()[0], outer_iter=-1, dtype=np.float64)
    assert I.dtype == np.float64
    worst = 0.0
    for it in range(ref.iterations(5)):
        nxt = ref.outer_iteration(I, 25, np.float64)
        for k in range(I.shape[2]):
            s0, s1 = I[:, :, k].sum(), nxt[:, :, k].sum()
            rel = abs(s1 - s0) / abs(s0)
            print("iteration %d channel %d: relative change of the sum %.3g" % (it, k, rel))
            worst = max(worst, rel)
            assert rel <= 1e-9, (it, k, rel)
        I = nxt
    assert not np.array_equal(I, drivsco()[0].astype(np.float64))  # the image did change
    print("worst %.3g" % worst)


# ---- degenerate parameters ----------------------------------------------------------------------------------------------------

def test_alpha_zero_returns_the_input():
    """alpha = 0: b = 2 and a = c = 0, so ver = hor = d/2 exactly and their sum is d."""
    I = drivsco()[0]
    _eq(ref.Diffusion4_v10(I, alpha=0, outer_iter=2), I, "alpha = 0")


def test_outer_iter_counts_like_the_matlab_loop():
    I = gray()
    assert [ref.iterations(k) for k in (-1, -0.5, 0, 0.5, 2, 2.5, 5)] == [0, 0, 1, 1, 3, 3, 6]
    _eq(ref.Diffusion4_v10(I, outer_iter=-1), I, "outer_iter = -1")
    _eq(ref.Diffusion4_v10(I, outer_iter=2.5), ref.Diffusion4_v10(I, outer_iter=2), "outer_iter = 2.5 vs 2")
    assert not pb.bit_equal(ref.Diffusion4_v10(I, outer_iter=0), I)


# ---- uint8 --------------------------------------------------------------------------------------------------------------------

UINT8_CASES = [(2.5, 3), (3.5, 4), (-0.4, 0), (255.6, 255), (np.inf, 255), (-np.inf, 0), (np.nan, 0), (0.49999997, 0),
               (254.5, 255), (-0.5, 0), (1e9, 255), (7.0, 7)]


def test_uint8_follows_matlab(pdeip):
    drv = importlib.import_module("pde-based-image-processing_amd.drivers")
    x = np.array([v for v, _ in UINT8_CASES], F32)
    want = np.array([w for _, w in UINT8_CASES], np.uint8)
    for fn in (drv.uint8_matlab, ref.to_uint8):
        got = fn(x)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (fn.__name__, got, want)


# ---- the boundary -------------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_entries(pdeip):
    syms = declared_symbols()
    lib = ctypes.CDLL(pdeip.capi.LIB_PATH)
    for name in ENTRIES:
        assert name in syms, name
        assert hasattr(lib, name), name
        assert name in pdeip.capi.SIGNATURES, name


def _prm(pdeip, alpha, outer_iter):
    dev = importlib.import_module("pde-based-image-processing_amd.device")
    return dev.Diffusion4Params(alpha, outer_iter)


REFUSED = [((1, 5, 1), (25.0, 5.0), "at least 2x2"), ((5, 1, 3), (25.0, 5.0), "at least 2x2"), ((1, 1, 1), (25.0, 5.0), "at least 2x2"),
           ((4, 4, 0), (25.0, 5.0), "channels"), ((4, 4, 1), (np.inf, 5.0), "alpha"), ((4, 4, 1), (-np.inf, 5.0), "alpha"),
           ((4, 4, 1), (1e39, 5.0), "alpha"), ((4, 4, 3), (25.0, np.inf), "outer_iter"), ((4, 4, 3), (25.0, -np.inf), "outer_iter"),
           ((2, 65536, 1), (25.0, 5.0), "more than 65535 columns"), ((2, 2, 65536), (25.0, 5.0), "more than 65535 channels")]
# the column is blockIdx.y of the weight kernel and the channel blockIdx.y of the line kernel: the launch geometry's refusals
UNSUPPORTED = ("more than 65535 columns", "more than 65535 channels")


@pytest.mark.parametrize("shape,params,msg", REFUSED)
def test_c_abi_refuses_without_a_gpu(pdeip, shape, params, msg):
    capi = pdeip.capi
    lib = capi.load()
    z = np.zeros(max(1, shape[0] * shape[1] * max(shape[2], 1)), F32)
    o = np.zeros_like(z)
    prm = _prm(pdeip, *params)
    code = capi.PDEIP_ERR_UNSUPPORTED if msg in UNSUPPORTED else capi.PDEIP_ERR_ARG
    rc = lib.pdeip_diffusion4(z.ctypes.data, shape[0], shape[1], shape[2], ctypes.addressof(prm), o.ctypes.data)
    assert rc == code and msg in capi.last_error(), capi.last_error()
    rc = lib.pdeip_diffusion4_dev(None, z.ctypes.data, shape[0], shape[1], shape[2], ctypes.addressof(prm), o.ctypes.data)
    assert rc == code and msg in capi.last_error(), capi.last_error()


def test_c_abi_refuses_null_pointers(pdeip):
    capi = pdeip.capi
    lib = capi.load()
    z = np.zeros(16, F32)
    assert lib.pdeip_diffusion4(None, 4, 4, 1, None, z.ctypes.data) == capi.PDEIP_ERR_ARG
    assert lib.pdeip_diffusion4_dev(None, z.ctypes.data, 4, 4, 1, None, None) == capi.PDEIP_ERR_ARG
    assert "NULL" in capi.last_error()


def test_python_driver_refuses_unknown_parameters_and_short_lines(pdeip):
    drv = importlib.import_module("pde-based-image-processing_amd.drivers")
    I = np.zeros((4, 5, 3), F32)
    with pytest.raises(TypeError, match="unknown parameter 'beta'"):
        drv.Diffusion4_v10(I, beta=1)
    with pytest.raises(TypeError, match="unknown parameter 'ITER'"):
        drv.Diffusion4_v10(I, ITER=3)
    with pytest.raises(pdeip.PdeipError, match="at least 2x2"):
        drv.Diffusion4_v10(np.zeros((1, 5), np.uint8))
    with pytest.raises(pdeip.PdeipError, match="alpha"):
        drv.Diffusion4_v10(I, alpha=float("inf"))


def test_stub_checks_arity_types_and_params(pdeip):
    lib = build_diff_stub("Diffusion4_v10_gpu", pdeip)
    I = np.zeros((5, 6, 3), F32)
    pv = np.array([np.nan, np.nan])
    err, _ = call(lib, 1, [I])
    assert err == "Diffusion4_v10_gpu parameter error: wrong number of input parameters!"
    err, _ = call(lib, 1, [I, pv, pv])
    assert err == "Diffusion4_v10_gpu parameter error: wrong number of input parameters!"
    err, _ = call(lib, 1, [I.astype(np.float64), pv])
    assert err == "Diffusion4_v10_gpu: 'I' must be a noncomplex single-valued matrix."
    for bad in (np.array([25.0]), np.array([25.0, 5.0, 1.0]), np.array([25, 5], F32)):
        err, _ = call(lib, 1, [I, bad])
        assert err == "Diffusion4_v10_gpu: 'params' must be a real double vector of 2 elements", bad
    err, _ = call(lib, 0, [I, pv])
    assert err == "Diffusion4_v10_gpu insufficient number of outputs. Output from this function is 'Iout'"
    err, _ = call(lib, 1, [np.zeros((1, 6, 3), F32), pv])
    assert "at least 2x2" in err  # refused by the library before any HIP call
    err, _ = call(lib, 1, [I, np.array([np.inf, 5.0])])
    assert "alpha" in err
