"""CPU: the MEX entry of the hole filling (pde-based-image-processing_amd/mex/denoising/TVinpaint4_gpu.c) compiles against the mock MEX
runtime (tests/mexmock) with -Wall -Wextra -Werror, and its argument checks fire before anything touches the GPU.  The GPU half is
in tests/test_gpu_inpaint.py."""
import ctypes
import os
import subprocess

import numpy as np

from test_flowviz_stub import BUILD_DIR, MOCK_DIR, ROOT, call_typed
from test_mex_stubs import to_mx

F32, F64 = np.float32, np.float64
SRC_DIR = os.path.join(ROOT, "pde-based-image-processing_amd", "mex", "denoising")
PARAMS = np.array([5.0, 1.75, 10, 5, 2, 0.75, 16, 0.25, 20.0, 1.0])


def build_inpaint_stub(pdeip):
    """Compile mex/denoising/TVinpaint4_gpu.c against the mock MEX runtime and libpdeip.so."""
    os.makedirs(BUILD_DIR, exist_ok=True)
    so = os.path.join(BUILD_DIR, "denoising_TVinpaint4_gpu.so")
    srcs = [os.path.join(SRC_DIR, "TVinpaint4_gpu.c"), os.path.join(MOCK_DIR, "mexmock.c")]
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
    names = ("alpha", "omega", "outer_iter", "inner_iter", "solver", "scl_factor", "min_size", "cover", "guide_scale", "keep")
    pv = PARAMS.copy()
    for k, v in kw.items():
        pv[names.index(k)] = v
    return pv


def test_stub_checks_arity_class_shape_and_parameters(pdeip):
    lib = build_inpaint_stub(pdeip)
    D = np.zeros((20, 24), F32)
    none = np.zeros((0, 0), F64)
    both = (F32, F32)
    for args in ([D, none], [D, none, PARAMS, PARAMS]):
        err, _ = call_typed(lib, both, args)
        assert err == "TVinpaint4_gpu parameter error: wrong number of input parameters!"
    for outs in ((), (F32, F32, F32)):
        err, _ = call_typed(lib, outs, [D, none, PARAMS])
        assert err.startswith("TVinpaint4_gpu wrong number of outputs")
    err, _ = call_typed(lib, both, [np.zeros((20, 24, 2, 2), F32), none, PARAMS])
    assert err == "TVinpaint4_gpu: 'D' must be a [rows x cols (x frames)] array"
    for guide in (np.zeros((20, 25), F32), np.zeros((19, 24, 3), F64), np.zeros((20, 24, 1, 2), F32)):
        err, _ = call_typed(lib, both, [D, guide, PARAMS])
        assert err == "TVinpaint4_gpu: 'guide' must be a [rows x cols (x channels)] array on the frame of 'D'", guide.shape
    for bad in (PARAMS[:9], np.concatenate([PARAMS, [0.0]]), PARAMS.astype(F32)):
        err, _ = call_typed(lib, both, [D, none, bad])
        assert err == "TVinpaint4_gpu: 'params' must be a real double vector of 10 elements"
    err, _ = call_typed(lib, both, [D, none, params(outer_iter=2.0 ** 31)])
    assert err == "TVinpaint4_gpu: a parameter is too large"
    for small in (np.zeros((2, 24), F32), np.zeros((20, 2), F64), np.zeros((0, 24), F32)):
        err, _ = call_typed(lib, both, [small, none, PARAMS])
        assert err == "TVinpaint4_gpu: 'D' must be at least 3x3", small.shape
    for solver in (3.0, 1.5):
        err, _ = call_typed(lib, both, [D, none, params(solver=solver)])
        assert err == "TVinpaint4_gpu: 'solver' must be 1 (point SOR) or 2 (line relaxation)"
    for scl in (1.0, 2.0, np.inf):
        for d in (D, D.astype(F64)):
            err, _ = call_typed(lib, both, [d, none, params(scl_factor=scl)])
            assert err == "TVinpaint4_gpu: 'scl_factor' must be below 1", scl
    err, _ = call_typed(lib, both, [D, D, params(cover=1.25)])
    assert err == "TVinpaint4_gpu: 'cover' must not be above 1"


def test_stub_refuses_other_classes(pdeip):
    """The mock runtime knows two classes; an array of a third one is neither single nor double."""
    lib = build_inpaint_stub(pdeip)
    dims = (20, 24)
    cd = (ctypes.c_long * 2)(*dims)
    raw = np.zeros(20 * 24, F64)
    good = np.zeros(dims, F32)
    for k, msg in ((0, "TVinpaint4_gpu: 'D' must be a noncomplex single or double array."),
                   (1, "TVinpaint4_gpu: 'guide' must be a noncomplex single or double array, or empty.")):
        args = [to_mx(lib, good), to_mx(lib, good), to_mx(lib, PARAMS)]
        lib.mock_free(args[k])
        args[k] = lib.mock_make(2, cd, 9, raw.ctypes.data)
        prhs = (ctypes.c_void_p * 3)(*args)
        plhs = (ctypes.c_void_p * 2)()
        assert lib.mock_call(2, plhs, 3, prhs) == 1
        assert lib.mock_last_error().decode() == msg
        for p in prhs:
            lib.mock_free(p)
