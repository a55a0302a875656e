"""CPU: the MEX entry of the frame interpolation (pde-based-image-processing_amd/mex/flow/flow_interpolate_gpu.c) compiles against the
mock MEX runtime (tests/mexmock) with -Wall -Wextra -Werror, and its argument checks fire before anything touches the GPU.  The GPU
half is in tests/test_gpu_interp.py."""
import ctypes

import numpy as np

from test_flowviz_stub import build_flow_stub, call_typed
from test_mex_stubs import to_mx

F32, F64 = np.float32, np.float64
OUT = (F32, F32, F32, F32)
NAMES = ("a", "b", "use_costs", "alpha", "omega", "outer_iter", "inner_iter", "solver", "scl_factor", "min_size", "cover", "guide_scale", "keep")
PARAMS = np.array([0.01, 0.5, 1.0, 5.0, 1.75, 10, 5, 2, 0.75, 16, 0.25, 20.0, 1.0])
NONE = np.zeros((0, 0), F64)
T = np.array([0.5])


def params(**kw):
    pv = PARAMS.copy()
    for k, v in kw.items():
        pv[NAMES.index(k)] = v
    return pv


def args(I0=None, I1=None, Uf=None, Vf=None, Ub=NONE, Vb=NONE, t=T, pv=PARAMS):
    img, plane = np.zeros((20, 24, 3), F32), np.zeros((20, 24), F32)
    pick = lambda given, dflt: dflt if given is None else given
    return [pick(I0, img), pick(I1, img), pick(Uf, plane), pick(Vf, plane), Ub, Vb, t, pv]


def test_stub_checks_arity_class_shape_and_parameters(pdeip):
    lib = build_flow_stub("flow_interpolate_gpu", pdeip)
    plane = np.zeros((20, 24), F32)
    for a in (args()[:7], args() + [PARAMS]):
        err, _ = call_typed(lib, OUT, a)
        assert err == "flow_interpolate_gpu parameter error: wrong number of input parameters!"
    for outs in ((), OUT + (F32,)):
        err, _ = call_typed(lib, outs, args())
        assert err.startswith("flow_interpolate_gpu wrong number of outputs")
    for a in (args(Ub=plane), args(Vb=plane)):
        err, _ = call_typed(lib, OUT, a)
        assert err == "flow_interpolate_gpu: 'Ub' and 'Vb' must both be given or both be []"
    err, _ = call_typed(lib, OUT, args(I0=np.zeros((20, 24, 3, 2), F32)))
    assert err == "flow_interpolate_gpu: 'I0' must be a [rows x cols (x channels)] array"
    for other in (np.zeros((20, 24), F32), np.zeros((20, 25, 3), F32), np.zeros((19, 24, 3), F64), np.zeros((20, 24, 3, 1, 2), F32)):
        err, _ = call_typed(lib, OUT, args(I1=other))
        assert err == "flow_interpolate_gpu: 'I0' and 'I1' must have one size", other.shape
    for bad in (np.zeros((20, 25), F32), np.zeros((19, 24), F64), np.zeros((20, 24, 2), F32)):
        for a in (args(Uf=bad), args(Vf=bad), args(Ub=bad, Vb=plane), args(Ub=plane, Vb=bad)):
            err, _ = call_typed(lib, OUT, a)
            assert err == "flow_interpolate_gpu: the flow planes must be [rows x cols] arrays on the frame of 'I0'", bad.shape
    for bad in (np.array([0.5, 0.5]), np.array([0.5], F32), np.zeros((0,))):
        err, _ = call_typed(lib, OUT, args(t=bad))
        assert err == "flow_interpolate_gpu: 't' must be a real double scalar"
    for bad in (0.0, 1.0, -0.5, 1.5, np.nan, np.inf):
        err, _ = call_typed(lib, OUT, args(t=np.array([bad])))
        assert err == "flow_interpolate_gpu: 't' must lie strictly between 0 and 1", bad
    for bad in (PARAMS[:12], np.concatenate([PARAMS, [0.0]]), PARAMS.astype(F32)):
        err, _ = call_typed(lib, OUT, args(pv=bad))
        assert err == "flow_interpolate_gpu: 'params' must be a real double vector of 13 elements"
    for kw in (dict(a=-0.01), dict(b=-0.5), dict(a=np.nan), dict(b=np.nan), dict(a=-np.inf)):
        err, _ = call_typed(lib, OUT, args(pv=params(**kw)))
        assert err == "flow_interpolate_gpu: 'a' and 'b' must be >= 0", kw
    err, _ = call_typed(lib, OUT, args(pv=params(outer_iter=2.0 ** 31)))
    assert err == "flow_interpolate_gpu: a parameter is too large"
    for rows, cols in ((2, 24), (20, 2), (0, 24)):
        small = args(I0=np.zeros((rows, cols), F32), I1=np.zeros((rows, cols), F32), Uf=np.zeros((rows, cols), F32), Vf=np.zeros((rows, cols), F64))
        err, _ = call_typed(lib, OUT, small)
        assert err == "flow_interpolate_gpu: the frames must be at least 3x3", (rows, cols)
    for solver in (3.0, 1.5):
        err, _ = call_typed(lib, OUT, args(pv=params(solver=solver)))
        assert err == "flow_interpolate_gpu: 'solver' must be 1 (point SOR) or 2 (line relaxation)"
    for scl in (1.0, 2.0, np.inf):
        err, _ = call_typed(lib, OUT, args(pv=params(scl_factor=scl)))
        assert err == "flow_interpolate_gpu: 'scl_factor' must be below 1", scl
    err, _ = call_typed(lib, OUT, args(pv=params(cover=1.25)))
    assert err == "flow_interpolate_gpu: 'cover' must not be above 1"


def test_stub_refuses_other_classes(pdeip):
    """The mock runtime knows two classes; an array of a third one is neither single nor double.  Empty Ub, Vb of any class pass."""
    lib = build_flow_stub("flow_interpolate_gpu", pdeip)
    plane = np.zeros((20, 24), F32)
    cd = (ctypes.c_long * 2)(20, 24)
    raw = np.zeros(20 * 24, F64)
    for k, name in enumerate(("I0", "I1", "Uf", "Vf", "Ub", "Vb")):
        a = [to_mx(lib, x) for x in args(I0=plane, I1=plane, Ub=plane, Vb=plane)]
        lib.mock_free(a[k])
        a[k] = lib.mock_make(2, cd, 9, raw.ctypes.data)
        prhs = (ctypes.c_void_p * 8)(*a)
        plhs = (ctypes.c_void_p * 4)()
        assert lib.mock_call(1, plhs, 8, prhs) == 1
        assert lib.mock_last_error().decode() == "flow_interpolate_gpu: '%s' must be a noncomplex single or double array." % name
        for p in prhs:
            lib.mock_free(p)
