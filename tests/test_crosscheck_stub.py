"""CPU: the MEX entries of the cross-checks (pde-based-image-processing_amd/mex/flow/disp_crosscheck_gpu.c, flow_crosscheck_gpu.c)
compile against the mock MEX runtime (tests/mexmock) with -Wall -Wextra -Werror, and their argument checks fire before anything touches
the GPU.  The GPU half is in tests/test_gpu_crosscheck.py."""
import ctypes

import numpy as np

from test_flowviz_stub import build_flow_stub, call_typed
from test_mex_stubs import to_mx

F32, F64 = np.float32, np.float64
DISP_OUT = (F32, F32, F64)
FLOW_OUT = (F32, F32, F64)


def test_disp_stub_checks_arity_class_shape_and_tol(pdeip):
    lib = build_flow_stub("disp_crosscheck_gpu", pdeip)
    D = np.zeros((5, 6), F32)
    tol = np.array([1.0])
    for args in ([D, D], [D, D, tol, tol]):
        err, _ = call_typed(lib, DISP_OUT, args)
        assert err == "disp_crosscheck_gpu parameter error: wrong number of input parameters!"
    for outs in ((), (F32, F32, F64, F64)):
        err, _ = call_typed(lib, outs, [D, D, tol])
        assert err.startswith("disp_crosscheck_gpu wrong number of outputs")
    for a, b in ((D, np.zeros((5, 7), F32)), (D, np.zeros((4, 6), F64)), (np.zeros((5, 6, 2), F32), np.zeros((5, 6, 2), F32)),
                 (D, np.zeros((5, 6, 1, 2), F32))):
        err, _ = call_typed(lib, DISP_OUT, [a, b, tol])
        assert err == "disp_crosscheck_gpu: 'D0' and 'D1' must be [rows x cols] arrays of one size", (a.shape, b.shape)
    for bad in (np.array([1.0, 2.0]), np.array([1.0], F32), np.zeros((0,))):
        err, _ = call_typed(lib, DISP_OUT, [D, D, bad])
        assert err == "disp_crosscheck_gpu: 'tol' must be a real double scalar"
    for bad in (-1.0, np.nan, -np.inf):
        for d in (D, D.astype(F64)):
            err, _ = call_typed(lib, DISP_OUT, [d, d, np.array([bad])])
            assert err == "disp_crosscheck_gpu: 'tol' must be >= 0", bad
    for small in (np.zeros((5, 1), F32), np.zeros((0, 6), F32)):
        err, _ = call_typed(lib, DISP_OUT, [small, small, tol])
        assert err == "disp_crosscheck_gpu: 'D0' must be at least 1x2"


def test_flow_stub_checks_arity_class_shape_and_parameters(pdeip):
    lib = build_flow_stub("flow_crosscheck_gpu", pdeip)
    flow = np.zeros((5, 6, 2), F32)
    pv = np.array([0.01, 0.5])
    for args in ([flow, flow], [flow, flow, pv, pv]):
        err, _ = call_typed(lib, FLOW_OUT, args)
        assert err == "flow_crosscheck_gpu parameter error: wrong number of input parameters!"
    for outs in ((), (F32, F32, F64, F64)):
        err, _ = call_typed(lib, outs, [flow, flow, pv])
        assert err.startswith("flow_crosscheck_gpu wrong number of outputs")
    for bad in (np.zeros((5, 6, 3), F32), np.zeros((5, 6), F32), np.zeros((5, 6, 1), F64), np.zeros((5, 6, 2, 2), F32)):
        for args in ([bad, flow, pv], [flow, bad, pv]):
            err, _ = call_typed(lib, FLOW_OUT, args)
            assert err == "flow_crosscheck_gpu: 'flowF' and 'flowB' must be [rows x cols x 2] arrays", bad.shape
    for other in (np.zeros((5, 7, 2), F32), np.zeros((4, 6, 2), F64)):
        err, _ = call_typed(lib, FLOW_OUT, [flow, other, pv])
        assert err == "flow_crosscheck_gpu: 'flowF' and 'flowB' must have one size"
    for bad in (np.array([1.0]), np.array([1.0, 0.0, 0.0]), np.array([1, 0], F32)):
        err, _ = call_typed(lib, FLOW_OUT, [flow, flow, bad])
        assert err == "flow_crosscheck_gpu: 'params' must be a real double vector of 2 elements"
    for bad in ([-0.01, 0.5], [0.01, -0.5], [np.nan, 0.5], [0.01, np.nan], [-np.inf, 0.5]):
        for f in (flow, flow.astype(F64)):
            err, _ = call_typed(lib, FLOW_OUT, [f, f, np.array(bad)])
            assert err == "flow_crosscheck_gpu: 'a' and 'b' must be >= 0", bad
    for small in (np.zeros((1, 6, 2), F32), np.zeros((5, 1, 2), F32), np.zeros((0, 6, 2), F32)):
        err, _ = call_typed(lib, FLOW_OUT, [small, small, pv])
        assert err == "flow_crosscheck_gpu: the flows must be at least 2x2x2"


def test_stubs_refuse_other_classes(pdeip):
    """The mock runtime knows two classes; an array of a third one is neither single nor double."""
    for stub, dims, third, names in (("disp_crosscheck_gpu", (5, 6), np.array([1.0]), ("D0", "D1")),
                                     ("flow_crosscheck_gpu", (5, 6, 2), np.array([0.01, 0.5]), ("flowF", "flowB"))):
        lib = build_flow_stub(stub, pdeip)
        cd = (ctypes.c_long * len(dims))(*dims)
        raw = np.zeros(int(np.prod(dims)), F64)
        good = np.zeros(dims, F32)
        for k in range(2):
            args = [to_mx(lib, good), to_mx(lib, good), to_mx(lib, third)]
            lib.mock_free(args[k])
            args[k] = lib.mock_make(len(dims), cd, 9, raw.ctypes.data)
            prhs = (ctypes.c_void_p * 3)(*args)
            plhs = (ctypes.c_void_p * 3)()
            assert lib.mock_call(3, plhs, 3, prhs) == 1
            assert lib.mock_last_error().decode() == "%s: '%s' must be a noncomplex single or double array." % (stub, names[k])
            for p in prhs:
                lib.mock_free(p)
