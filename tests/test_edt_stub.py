"""CPU: the MEX entry of bwdist (pde-based-image-processing_amd/mex/morph/bwdist_gpu.c) compiles against the mock MEX runtime
(tests/mexmock) with -Wall -Wextra -Werror, and its argument checks fire before anything touches the GPU.  The GPU half is in
tests/test_gpu_edt.py, which imports the helper below."""
import ctypes
import os
import subprocess

import numpy as np

from test_flowviz_stub import BUILD_DIR, call_typed
from test_mex_stubs import MOCK_DIR, ROOT, to_mx

F32, F64 = np.float32, np.float64
MORPH_DIR = os.path.join(ROOT, "pde-based-image-processing_amd", "mex", "morph")
OUT = (F32, F32)    # D, and IDX: uint32 words read as 4-byte singles (the mock's reader knows two classes); view them as uint32


def build_morph_stub(name, pdeip):
    """Compile mex/morph/<name>.c against the mock MEX runtime and libpdeip.so."""
    os.makedirs(BUILD_DIR, exist_ok=True)
    so = os.path.join(BUILD_DIR, "morph_" + name + ".so")
    srcs = [os.path.join(MORPH_DIR, name + ".c"), os.path.join(MOCK_DIR, "mexmock.c")]
    deps = srcs + [os.path.join(MORPH_DIR, "..", "pdeip_mex_util.h"), os.path.join(MOCK_DIR, "mex.h"), pdeip.capi.LIB_PATH]
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


def test_stub_checks_arity_class_and_shape(pdeip):
    lib = build_morph_stub("bwdist_gpu", pdeip)
    BW = np.zeros((5, 6), F32)
    for args in ([], [BW, BW]):
        err, _ = call_typed(lib, OUT, args)
        assert err == "bwdist_gpu parameter error: wrong number of input parameters!"
    for outs in ((), (F32, F32, F32)):
        err, _ = call_typed(lib, outs, [BW])
        assert err.startswith("bwdist_gpu wrong number of outputs")
    for bad in (np.zeros((5, 6, 2), F32), np.zeros((5, 6, 1, 2), F64)):
        err, _ = call_typed(lib, OUT, [bad])
        assert err == "bwdist_gpu: 'BW' must be a [rows x cols] array", bad.shape
    for small in (np.zeros((0, 6), F32), np.zeros((5, 0), F64)):
        err, _ = call_typed(lib, OUT, [small])
        assert err == "bwdist_gpu: 'BW' must be at least 1x1"
    err, _ = call_typed(lib, OUT, [np.zeros((32768, 1), F32)])     # the library's own refusal, handed on before any HIP call
    assert "32767" in err and "pdeip_bwdist" in err


def test_stub_refuses_other_classes(pdeip):
    """The mock runtime knows two classes; an array of a third one is neither single nor double."""
    lib = build_morph_stub("bwdist_gpu", pdeip)
    dims = (ctypes.c_long * 2)(5, 6)
    raw = np.zeros(5 * 6, F64)
    prhs = (ctypes.c_void_p * 1)(lib.mock_make(2, dims, 9, raw.ctypes.data))
    plhs = (ctypes.c_void_p * 2)()
    assert lib.mock_call(2, plhs, 1, prhs) == 1
    assert lib.mock_last_error().decode() == "bwdist_gpu: 'BW' must be a noncomplex single or double array."
    lib.mock_free(prhs[0])
