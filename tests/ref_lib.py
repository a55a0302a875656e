"""ctypes access to the reference's own MEX gateways, built unchanged into oracle/_ref/<Gateway>.so by
oracle/build_ref.py against the stand-in MEX runtime oracle/refmex/.

TEST INFRASTRUCTURE.  `call(gateway, nlhs, *args)` calls a gateway's mexFunction as MATLAB does: every argument becomes
a fresh mxArray (float32 -> single, anything else -> double; scalars 1x1), outputs come back with the dimensions the
gateway created them with, and an error the gateway raises through mexErrMsgTxt raises RefMexError(message).

Only oracle/_ref/ is read here, never the reference tree: the build travels with the working tree, the reference does not.
"""
import ctypes
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
MANIFEST = os.path.join(REF_DIR, "MANIFEST.json")
SINGLE, DOUBLE = 7, 6

_libs = {}


class RefMexError(Exception):
    """The gateway called mexErrMsgTxt; args[0] is its message."""


def manifest():
    try:
        with open(MANIFEST) as f:
            return json.load(f)
    except (OSError, ValueError):
        return None


def available():
    """The manifest, when oracle/_ref/ holds a complete build made from the stand-in runtime in this tree; else None.
    (Whether it is current against the reference's sources is oracle/build_ref.py's up_to_date().)"""
    import importlib.util

    m = manifest()
    if m is None or not all(os.path.exists(os.path.join(REF_DIR, g + ".so")) for g in m.get("gateways", ())):
        return None
    spec = importlib.util.spec_from_file_location("pdeip_build_ref", os.path.join(ROOT, "oracle", "build_ref.py"))
    br = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(br)
    return m if m.get("stand_in_sha256") == br.stand_in_hashes() else None


def lib(gateway):
    if gateway not in _libs:
        so = os.path.join(REF_DIR, gateway + ".so")
        if not os.path.exists(so):
            raise FileNotFoundError("%s is not built (oracle/build_ref.py)" % so)
        L = ctypes.CDLL(so)
        L.refmex_make.restype = ctypes.c_void_p
        L.refmex_make.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_longlong), ctypes.c_void_p]
        L.refmex_free.argtypes = [ctypes.c_void_p]
        L.refmex_class.argtypes = [ctypes.c_void_p]
        L.refmex_ndim.argtypes = [ctypes.c_void_p]
        L.refmex_dim.restype = ctypes.c_longlong
        L.refmex_dim.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.refmex_data.restype = ctypes.c_void_p
        L.refmex_data.argtypes = [ctypes.c_void_p]
        L.refmex_error.restype = ctypes.c_char_p
        L.refmex_call.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        _libs[gateway] = L
    return _libs[gateway]


def mwsize_bytes(gateway):
    """sizeof(mwSize) in the stand-in runtime linked into `gateway`."""
    return lib(gateway).refmex_mwsize_bytes()


def _to_mx(L, a):
    a = np.asarray(a)
    if a.dtype != np.float32:
        a = a.astype(np.float64)
    a = np.asfortranarray(a.reshape(1, 1) if a.ndim == 0 else a)
    dims = (ctypes.c_longlong * a.ndim)(*a.shape)
    p = L.refmex_make(SINGLE if a.dtype == np.float32 else DOUBLE, a.ndim, dims, a.ctypes.data)
    if not p:
        raise MemoryError("refmex_make failed for shape %s" % (a.shape,))
    return p


def _from_mx(L, p):
    shape = tuple(L.refmex_dim(p, k) for k in range(L.refmex_ndim(p)))
    dt = np.float32 if L.refmex_class(p) == SINGLE else np.float64
    n = int(np.prod(shape))
    buf = np.ctypeslib.as_array(ctypes.cast(L.refmex_data(p), ctypes.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(max(n, 1),))
    return buf[:n].copy().reshape(shape, order="F")


def call(gateway, nlhs, *args, return_inputs=False):
    """[out1, ..., out_nlhs] = gateway(args...).  Each argument is passed as a copy.  Returns the list of outputs (None where
    the gateway created none), or (outputs, inputs after the call) with return_inputs=True."""
    L = lib(gateway)
    prhs = (ctypes.c_void_p * max(len(args), 1))()
    plhs = (ctypes.c_void_p * max(nlhs, 1))()
    try:
        for k, a in enumerate(args):
            prhs[k] = _to_mx(L, a)
        rc = L.refmex_call(int(nlhs), plhs, len(args), prhs)
        if rc:
            raise RefMexError(L.refmex_error().decode())
        outs = [_from_mx(L, plhs[k]) if plhs[k] else None for k in range(max(nlhs, 1))]
        if return_inputs:
            return outs, [_from_mx(L, prhs[k]) for k in range(len(args))]
        return outs
    finally:
        for p in list(prhs) + list(plhs):
            if p:
                L.refmex_free(p)
