"""CPU: the MEX entry of primal-dual total variation (pde-based-image-processing_amd/mex/denoising/TVdenoisePD_gpu.c) compiles against
the mock MEX runtime (tests/mexmock) with -Wall -Wextra -Werror, its argument checks fire before anything touches the GPU, and the
library's own refusals come back as its error text.  The GPU half is in tests/test_gpu_tvpd.py, which imports the helper below."""
import ctypes
import os
import subprocess

import numpy as np

from test_flowviz_stub import BUILD_DIR, MOCK_DIR, ROOT, call_typed
from test_mex_stubs import to_mx

F32, F64 = np.float32, np.float64
SRC_DIR = os.path.join(ROOT, "pde-based-image-processing_amd", "mex", "denoising")
NAMES = ("model", "lambda", "huber", "iter", "tau", "sigma")
PARAMS = np.array([0.0, 0.8, 0.0, 10.0, np.nan, np.nan])
NONE = np.zeros((0, 0), F64)
OUT = (F32,)


def build_tvpd_stub(pdeip):
    """Compile mex/denoising/TVdenoisePD_gpu.c against the mock MEX runtime and libpdeip.so."""
    os.makedirs(BUILD_DIR, exist_ok=True)
    so = os.path.join(BUILD_DIR, "denoising_TVdenoisePD_gpu.so")
    srcs = [os.path.join(SRC_DIR, "TVdenoisePD_gpu.c"), os.path.join(MOCK_DIR, "mexmock.c")]
    deps = srcs + [os.path.join(SRC_DIR, "..", "pdeip_mex_util.h"), os.path.join(MOCK_DIR, "mex.h"), pdeip.capi.LIB_PATH]
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


def params(**kw):
    pv = PARAMS.copy()
    for k, v in kw.items():
        pv[NAMES.index(k)] = v
    return pv


def test_stub_checks_arity_class_shape_and_parameters(pdeip):
    lib = build_tvpd_stub(pdeip)
    I = np.zeros((5, 6), F32)
    for args in ([I, NONE], [I, NONE, PARAMS, PARAMS]):
        err, _ = call_typed(lib, OUT, args)
        assert err == "TVdenoisePD_gpu parameter error: wrong number of input parameters!"
    for outs in ((), (F32, F32)):
        err, _ = call_typed(lib, outs, [I, NONE, PARAMS])
        assert err.startswith("TVdenoisePD_gpu wrong number of outputs")
    err, _ = call_typed(lib, OUT, [np.zeros((5, 6, 2, 2), F32), NONE, PARAMS])
    assert err == "TVdenoisePD_gpu: 'I' must be a [rows x cols (x frames)] array"
    for small in (np.zeros((0, 6), F32), np.zeros((5, 0), F64)):
        err, _ = call_typed(lib, OUT, [small, NONE, PARAMS])
        assert err == "TVdenoisePD_gpu: 'I' must be at least 1x1", small.shape
    for u0 in (np.zeros((5, 7), F32), np.zeros((4, 6), F64), np.zeros((5, 6, 2), F32), np.zeros((5, 6, 1, 2), F32)):
        err, _ = call_typed(lib, OUT, [I, u0, PARAMS])
        assert err == "TVdenoisePD_gpu: 'u0' must have the size of 'I'", u0.shape
    for bad in (PARAMS[:5], np.concatenate([PARAMS, [0.0]]), PARAMS.astype(F32)):
        err, _ = call_typed(lib, OUT, [I, NONE, bad])
        assert err == "TVdenoisePD_gpu: 'params' must be a real double vector of 6 elements"
    for model in (2.0, -1.0, 0.5, np.nan):
        err, _ = call_typed(lib, OUT, [I, NONE, params(model=model)])
        assert err == "TVdenoisePD_gpu: 'model' must be 0 (TV-L1) or 1 (ROF)", model
    for it in (-1.0, 2.5, np.nan, np.inf, 2.0 ** 31):
        for i in (I, I.astype(F64)):
            err, _ = call_typed(lib, OUT, [i, NONE, params(iter=it)])
            assert err == "TVdenoisePD_gpu: 'iter' must be a non-negative integer", it


def test_stub_forwards_its_arguments_to_the_library(pdeip):
    """What the stub does not check itself reaches pdeip_tv_pd, whose refusals fire before any HIP call: each parameter lands in its
    member."""
    lib = build_tvpd_stub(pdeip)
    I = np.zeros((5, 6, 2), F64)
    for kw, text in ((dict(**{"lambda": -1.0}), "lambda must be finite and >= 0 (got -1)"), (dict(huber=np.inf), "huber must be finite and >= 0 (got inf)"),
                     (dict(tau=-0.25), "tau must be positive and finite (got -0.25)"), (dict(sigma=0.0), "sigma must be positive and finite (got 0)"),
                     (dict(tau=0.5), "tau * sigma * 8 must not exceed 1 (got 2)"), (dict(tau=0.25, sigma=0.75), "must not exceed 1 (got 1.5)")):
        err, _ = call_typed(lib, OUT, [I, I.astype(F32), params(**kw)])
        assert err is not None and "pdeip_tv_pd:" in err and text in err, (kw, err)
    err, _ = call_typed(lib, OUT, [np.zeros((1, 65536), F32), NONE, PARAMS])
    assert "pdeip_tv_pd:" in err and "65535" in err


def test_stub_refuses_other_classes(pdeip):
    """The mock runtime knows two classes; an array of a third one is neither single nor double."""
    lib = build_tvpd_stub(pdeip)
    cd = (ctypes.c_long * 2)(5, 6)
    raw = np.zeros(5 * 6, F64)
    good = np.zeros((5, 6), F32)
    for k, msg in ((0, "TVdenoisePD_gpu: 'I' must be a noncomplex single or double array."),
                   (1, "TVdenoisePD_gpu: 'u0' must be a noncomplex single or double array, or empty.")):
        args = [to_mx(lib, good), to_mx(lib, good), to_mx(lib, PARAMS)]
        lib.mock_free(args[k])
        args[k] = lib.mock_make(2, cd, 9, raw.ctypes.data)
        prhs = (ctypes.c_void_p * 3)(*args)
        plhs = (ctypes.c_void_p * 1)()
        assert lib.mock_call(1, plhs, 3, prhs) == 1
        assert lib.mock_last_error().decode() == msg
        for p in prhs:
            lib.mock_free(p)
