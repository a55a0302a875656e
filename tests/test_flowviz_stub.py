"""CPU: the MEX entry of flow2color (pde-based-image-processing_amd/mex/flow/flow2color_gpu.c) compiles against the mock MEX runtime
(tests/mexmock) with -Wall -Wextra -Werror, and its argument checks fire before anything touches the GPU.  The GPU half is in
tests/test_gpu_flowviz.py, which imports the helpers below."""
import ctypes
import os
import subprocess

import numpy as np

from test_mex_stubs import MOCK_DIR, ROOT, to_mx

F32 = np.float32
FLOW_DIR = os.path.join(ROOT, "pde-based-image-processing_amd", "mex", "flow")
BUILD_DIR = os.path.join(MOCK_DIR, "_build")


def build_flow_stub(name, pdeip):
    """Compile mex/flow/<name>.c against the mock MEX runtime and libpdeip.so."""
    os.makedirs(BUILD_DIR, exist_ok=True)
    so = os.path.join(BUILD_DIR, "flow_" + name + ".so")
    srcs = [os.path.join(FLOW_DIR, name + ".c"), os.path.join(MOCK_DIR, "mexmock.c")]
    deps = srcs + [os.path.join(FLOW_DIR, "..", "pdeip_mex_util.h"), os.path.join(MOCK_DIR, "mex.h"), pdeip.capi.LIB_PATH]
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


def call_typed(lib, out_types, args):
    """test_mex_stubs.call for outputs of mixed class: out_types names each output's numpy type.  Returns (error or None, outputs)."""
    prhs = (ctypes.c_void_p * len(args))(*[to_mx(lib, a) for a in args])
    nlhs = len(out_types)
    plhs = (ctypes.c_void_p * max(nlhs, 1))()
    rc = lib.mock_call(nlhs, plhs, len(args), prhs)
    outs = []
    if rc == 0:
        for k, t in enumerate(out_types):
            shape = tuple(lib.mock_dim(plhs[k], d) for d in range(lib.mock_ndim(plhs[k])))
            n = int(np.prod(shape))
            ctype = ctypes.c_float if t == np.float32 else ctypes.c_double
            buf = np.ctypeslib.as_array(ctypes.cast(lib.mock_data(plhs[k]), ctypes.POINTER(ctype)), shape=(n,)).copy()
            outs.append(buf.reshape(shape, order="F"))
    for p in list(prhs) + [q for q in plhs if q]:
        lib.mock_free(p)
    return (lib.mock_last_error().decode() if rc else None), outs


def test_stub_checks_arity_class_shape_and_border(pdeip):
    lib = build_flow_stub("flow2color_gpu", pdeip)
    flow = np.zeros((5, 6, 2), F32)
    pv = np.array([np.nan, 0.0])
    both = (np.float32, np.float64)
    for args in ([flow], [flow, pv, pv]):
        err, _ = call_typed(lib, both, args)
        assert err == "flow2color_gpu parameter error: wrong number of input parameters!"
    err, _ = call_typed(lib, (), [flow, pv])
    assert err.startswith("flow2color_gpu insufficient number of outputs")
    for bad in (np.zeros((5, 6, 3), F32), np.zeros((5, 6), F32), np.zeros((5, 6, 1), np.float64), np.zeros((5, 6, 2, 2), F32)):
        err, _ = call_typed(lib, both, [bad, pv])
        assert err == "flow2color_gpu: 'flow' must be a [rows x cols x 2] array", bad.shape
    for bad in (np.array([1.0]), np.array([1.0, 0.0, 0.0]), np.array([1, 0], F32)):
        err, _ = call_typed(lib, both, [flow, bad])
        assert err == "flow2color_gpu: 'params' must be a real double vector of 2 elements"
    for border in (-1.0, 2.5, np.nan, np.inf, 2.0 ** 31):
        for f in (flow, flow.astype(np.float64)):
            err, _ = call_typed(lib, both, [f, np.array([np.nan, border])])
            assert err == "flow2color_gpu: 'border' must be a non-negative integer", border
    err, _ = call_typed(lib, both, [np.zeros((0, 6, 2), F32), pv])
    assert err == "flow2color_gpu: 'flow' must be at least 1x1x2"


def test_stub_refuses_other_classes(pdeip):
    """The mock runtime knows two classes; an array of a third one is neither single nor double."""
    lib = build_flow_stub("flow2color_gpu", pdeip)
    dims = (ctypes.c_long * 3)(5, 6, 2)
    raw = np.zeros(5 * 6 * 2, np.float64)
    prhs = (ctypes.c_void_p * 2)(lib.mock_make(3, dims, 9, raw.ctypes.data), to_mx(lib, np.array([np.nan, 0.0])))
    plhs = (ctypes.c_void_p * 2)()
    assert lib.mock_call(2, plhs, 2, prhs) == 1
    assert lib.mock_last_error().decode() == "flow2color_gpu: 'flow' must be a noncomplex single or double array."
    for p in prhs:
        lib.mock_free(p)
