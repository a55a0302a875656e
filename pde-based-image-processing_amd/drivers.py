"""The MATLAB drivers as Python functions: same names, arguments and default parameters, every pyramid level resident on the
device (flow_level.py, fas.py) and so is the pyramid around them (pyramid.py states our definitions of imresize / imfilter /
fspecial, there being no IPT to compare with; csrc/pdeip_pyr.hpp computes exactly those): the frames go up once, the result
comes down once.  Inputs and outputs are MATLAB-shaped numpy arrays ([nrows, ncols(, C)],
images in 0..255 as the drivers expect); `mode` selects the ordering (capi.MODE_EXACT_ORDER reproduces the reference's order,
capi.MODE_RED_BLACK the parallel one).

    FlowEminND_llin_2D_v10      matlab/optical_flow/FlowEminND_llin_2D_v10.m      isotropic late-linearisation flow
    FlowEminAD_llin_2D_v10      matlab/optical_flow/FlowEminAD_llin_2D_v10.m      anisotropic diffusion
    FlowEminHS_elin_2D_v10      matlab/optical_flow/FlowEminHS_elin_2D_v10.m      Horn-Schunck, early linearisation
    FlowEminNDFASFMG_elin_2D_v10 matlab/optical_flow/FlowEminNDFASFMG_elin_2D_v10.m FAS full multigrid
    DispEminND_llin_2D          matlab/disparity/DispEminND_llin_2D.m             stereo disparity
    DispEminND_llin_sym_2D      matlab/disparity/DispEminND_llin_sym_2D.m         symmetric stereo
    TVdenoise8 / TVdenoise4     matlab/denoising/TVdenoise{8,4}.m                 total-variation denoising
    GAC_v10a / GAC_v10b         matlab/active_contour/GAC_v10{a,b}.m              geodesic active contours (C++ only: pdeip_gac)
    Diffusion4_v10              matlab/diffusion/Diffusion4_v10.m                 nonlinear diffusion (C++ only: pdeip_diffusion4)
    regionCompetition           matlab/segmentation/DispSegmentation.m:448-654    region competition of the segmentation drivers
    segments_numbered           matlab/segmentation/DispSegmentation.m:190-198    (C++ only: pdeip_region_competition, pdeip_seg_label)
    flow2color / flow_errors    matlab/optical_flow/flow2color.m                  colour coding; error measures (C++ only: pdeip_flow2color)
    disp_crosscheck / flow_crosscheck / stereo_maps   this library's own: left-right and forward-backward checks (pdeip_disp_crosscheck)
    TVinpaint4                  this library's own: the holes of a sparse map filled by TV inpainting (pdeip_tv_inpaint4)
    gaussian / Diffusion8       this library's own: smoothing at a chosen scale; structure-tensor diffusion, EED and CED (pdeip_diffusion8)
    bwdist / signed_distance / nearest_fill   this library's own: exact Euclidean distance transform (pdeip_bwdist, pdeip_signed_distance, pdeip_nearest_fill)
    TVdenoisePD                 this library's own: primal-dual total variation, TV-L1 / ROF / Huber-TV (pdeip_tv_pd)
    FlowTVL1                    this library's own: TV-L1 optical flow, primal-dual, warped, coarse to fine (pdeip_flow_tvl1)

`Us=`, `Vs=` (param.Us / param.Vs: spatial a-priori fields, double, NaN = no constraint) and `scales=` (param.scales) are taken
by the late-linearisation flow drivers and the disparity driver as the reference's drivers take them.
All eight also exist behind the C-ABI (pdeip_flow_nd_llin, pdeip_flow_ad_llin, pdeip_flow_hs_elin, pdeip_flow_fas_fmg_elin,
pdeip_disp_nd_llin, pdeip_disp_nd_llin_sym, pdeip_tvdenoise8 / 4: csrc/pdeip_drivers.hip) for callers that are not Python -- the
MATLAB session the toolbox runs in; the `capi_*` functions at the end of this file call those.
`graph=True` (the llin flow drivers and the FAS driver, parallel orderings): the run's launches are captured into a HIP graph
on the first call for a frame size and replayed afterwards (graphs.py) -- same kernels and bits, no per-launch host work.
"""
import contextlib
import ctypes
import math

import numpy as np
import torch

from . import capi, device as dev, fas, flow_level as fl, graphs, pyramid


def _up(t, inv, nrows, ncols, method="bilinear"):
    """imresize(t.*inv, [nrows ncols], method) on the device"""
    return dev.pyr_resize(t * np.float32(inv), nrows, ncols, method)


def _zeros_like_plane(t):
    return torch.zeros(t.shape[-2:], dtype=torch.float32, device=t.device)


def _frames(Iin, channels):
    """cat(3, frame0, frame1) -> the two frames on the device, [C, ncols, nrows] each (one upload, sliced there)."""
    I = np.asarray(Iin, dtype=np.float32)
    d = dev.to_device(I if I.ndim == 3 else I[:, :, None])
    return d[:channels].contiguous(), d[channels:2 * channels].contiguous()


def _c3(I):
    I = np.asarray(I, dtype=np.float32)
    return dev.to_device(I if I.ndim == 3 else I[:, :, None])


def _terms(d0, d1, fst, snd):
    """First / second constancy images of one scale on the device (:133-170 of the ND driver)."""
    fst, snd = fst.upper(), snd.upper()
    if fst not in ("RGB", "GRAD") or snd not in ("NONE", "RGB", "GRADMAG"):
        raise ValueError("No such fstTerm / sndTerm")
    I1 = (d0, d1) if fst == "RGB" else (dev.rgb2grad(d0), dev.rgb2grad(d1))
    I2 = (None, None) if snd == "NONE" else (d0, d1)
    return I1, I2


_GRAPHS = {}   # (driver, frame shape, parameters) -> graphs.GraphedRun of its device part


def _apriori_pyramid(field, shapes, scl_factor):
    """param.Us down the pyramid (FlowEminND_llin_2D_v10.m:162-184): NaN -> 0, USap{scl} = imresize(USap{scl-1} .* scl_factor), doubles.
    shapes: (rows, cols) per scale.  Returns the host arrays (finest first)."""
    us = np.array(field, dtype=np.float64)
    us[np.isnan(us)] = 0.0
    out = [us]
    for rows, cols in shapes[1:]:
        out.append(pyramid.resize(out[-1] * scl_factor, rows, cols, "bilinear", out_dtype=np.float64))
    return out


def _flow_llin_planes(level_cls, f0, f1, fstTerm, sndTerm, p, mode, Us=None, Vs=None, scales=None):
    """The level loop of the llin flow drivers on resident frames f0, f1 [C, ncols, nrows] (already ./255): the flow as two resident
    planes [ncols, nrows]; nothing is downloaded."""
    P0, P1 = pyramid.build_dev(f0, f1, p["scl_factor"], 20, max_scales=scales)
    level = level_cls(p, mode=mode)
    U = _zeros_like_plane(P0[-1])
    V = torch.zeros_like(U)
    shapes = [(t.shape[-1], t.shape[-2]) for t in P0]
    ap = {}
    for name, field in (("Us", Us), ("Vs", Vs)):
        if field is not None:
            ap[name] = _apriori_pyramid(field, shapes, p["scl_factor"])
    if "Us" in ap:   # U = USap{scales} (:178): MATLAB's double array; here its float32 rounding, as in the disparity driver
        U = dev.to_device(ap["Us"][-1].astype(np.float32))
    if "Vs" in ap:
        V = dev.to_device(ap["Vs"][-1].astype(np.float32))
    for scl in range(len(P0) - 1, -1, -1):
        d0, d1 = P0[scl], P1[scl]
        (a0, a1), (b0, b1) = _terms(d0, d1, fstTerm, sndTerm)
        args = (a0, a1, U, V) + ((d0,) if level_cls is fl.FlowAdLevel else ()) + (b0, b1)
        kw = {}
        if ap:
            on_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a.T)).to(U.device)
            kw = dict(Us=on_dev(ap["Us"][scl]) if "Us" in ap else None, Vs=on_dev(ap["Vs"][scl]) if "Vs" in ap else None,
                      as_diff=2.0 * p["scl_factor"] ** scl, u_double=(scl == len(P0) - 1))
        U, V = level.run(*args, **kw)
        if scl > 0:
            cols, rows = P0[scl - 1].shape[-2:]
            U, V = _up(U, 1.0 / p["scl_factor"], rows, cols), _up(V, 1.0 / p["scl_factor"], rows, cols)
    return U, V


def _flow_llin(level_cls, Iin, channels, fstTerm, sndTerm, defaults, mode, param):
    param = dict(param)
    graph = bool(param.pop("graph", False))   # exact order too since round 3: the walkers' schedule table is built on the stream
    Us, Vs, scales = param.pop("Us", None), param.pop("Vs", None), param.pop("scales", None)
    p = dict(defaults, **param)
    p["sndTerm"] = sndTerm.lower()
    I0, I1 = _frames(Iin, channels)
    if (Us is not None or Vs is not None) and graph:
        raise ValueError("graph=True replays a captured run: not with a-priori fields")

    def device_part(f0, f1):
        return _flow_llin_planes(level_cls, f0, f1, fstTerm, sndTerm, p, mode, Us, Vs, scales)

    f0, f1 = dev.div_scalar(I0, 255.0), dev.div_scalar(I1, 255.0)
    if graph:   # the few thousand launches of the run replayed as one HIP graph (graphs.py); same kernels, same results
        key = (level_cls.__name__, tuple(I0.shape), fstTerm.lower(), sndTerm.lower(), int(mode), scales, tuple(sorted((k, repr(v)) for k, v in p.items())))
        if key not in _GRAPHS:
            _GRAPHS[key] = graphs.GraphedRun(device_part)
        U, V = _GRAPHS[key](f0, f1)
    else:
        U, V = device_part(f0, f1)
    dev.sync_check()  # results leave the device: a timed-out dependency wait of the exact-order kernel must not pass silently
    return dev.to_matlab(U), dev.to_matlab(V)


ND_DEFAULTS = dict(alpha=0.042, omega=1.9, gammaS=0.01, firstLoop=4, secondLoop=4, iter=4, b1=1.4843, b2=0.2915, scl_factor=0.75, solver=2)
AD_DEFAULTS = dict(ND_DEFAULTS, quantile=0.9, diffusion="image")


def FlowEminND_llin_2D_v10(Iin, channels, fstTerm="rgb", sndTerm="none", mode=capi.MODE_EXACT_ORDER, **param):
    """[U V] = FlowEminND_llin_2D_v10(Iin, channels, fstTerm, sndTerm, ...): Iin = cat(3, frame0, frame1)."""
    return _flow_llin(fl.FlowLlinLevel, Iin, channels, fstTerm, sndTerm, ND_DEFAULTS, mode, param)


def FlowEminAD_llin_2D_v10(Iin, channels, fstTerm="rgb", sndTerm="none", mode=capi.MODE_EXACT_ORDER, **param):
    return _flow_llin(fl.FlowAdLevel, Iin, channels, fstTerm, sndTerm, AD_DEFAULTS, mode, param)


HS_DEFAULTS = dict(alpha=0.2, omega=1.9, iter=20, b1=0.25, b2=0.75, scl_factor=0.75, solver=2)


def FlowEminHS_elin_2D_v10(Iin, channels, mode=capi.MODE_EXACT_ORDER, **param):
    p = dict(HS_DEFAULTS, **param)
    I0, I1 = _frames(Iin, channels)
    P0, P1 = pyramid.build_dev(dev.div_scalar(I0, 255.0), dev.div_scalar(I1, 255.0), p["scl_factor"], 20)
    level = fl.FlowHsLevel(p, mode=mode)
    U = _zeros_like_plane(P0[-1])
    V = torch.zeros_like(U)
    for scl in range(len(P0) - 1, -1, -1):
        U, V = level.run(P0[scl], P1[scl], U, V)
        if scl > 0:   # imresize(medfilt2(U.*(1/scl_factor), [3 3], 'symmetric'), 'OutputSize', ...): the default, bicubic, method (:189-190)
            cols, rows = P0[scl - 1].shape[-2:]
            inv = np.float32(1.0 / p["scl_factor"])
            mU, mV = torch.empty_like(U), torch.empty_like(V)
            dev.median3(U * inv, None, mU)
            dev.median3(V * inv, None, mV)
            U, V = dev.pyr_resize(mU, rows, cols, "bicubic"), dev.pyr_resize(mV, rows, cols, "bicubic")
    dev.sync_check()  # results leave the device: a timed-out dependency wait of the exact-order kernel must not pass silently
    return dev.to_matlab(U), dev.to_matlab(V)


def FlowEminNDFASFMG_elin_2D_v10(Iin, channels, mode=capi.MODE_EXACT_ORDER, **param):
    I0, I1 = _frames(Iin, channels)
    param = dict(param)
    if param.pop("graph", False):
        key = ("FasFmgFlow", tuple(I0.shape), int(mode), tuple(sorted((k, repr(v)) for k, v in param.items())))
        if key not in _GRAPHS:
            _GRAPHS[key] = fas.FasFmgFlow(param, mode=mode)
        gU, gV = _GRAPHS[key].run_graph(I0, I1)
    else:
        gU, gV = fas.FasFmgFlow(param, mode=mode).run(I0, I1)
    dev.sync_check()
    return dev.to_matlab(gU), dev.to_matlab(gV)


DISP_DEFAULTS = dict(alpha=0.042, gammaS=0.005, omega=1.9, firstLoop=4, secondLoop=6, iter=4, b1=1.48, b2=0.29, scl_factor=0.75, solver=2)   # DispEminND_llin_2D.m:51-63


def DispEminND_llin_2D(Il, Ir, fstTerm="rgb", sndTerm="none", mode=capi.MODE_EXACT_ORDER, Us=None, scales=None, **param):
    """Us: param.Us of the reference, a spatial a-priori disparity map at full resolution (double; NaN = no constraint there,
    zeroed as DispEminND_llin_2D.m:170 does).  It is scaled down with the pyramid (:172-176), starts the coarsest scale (:178;
    there MATLAB's U is that double array itself -- here its float32 rounding, a 1e-8 relative difference in the first
    firstLoop of the coarsest scale) and enters every assembly through the exp influence function (:277-292)."""
    p = dict(DISP_DEFAULTS, **param)
    p["sndTerm"] = sndTerm.lower()
    P0, P1 = pyramid.build_dev(dev.div_scalar(_c3(Il), 255.0), dev.div_scalar(_c3(Ir), 255.0), p["scl_factor"], 10, max_scales=scales)
    level = fl.DispLlinLevel(p, mode=mode)
    U = _zeros_like_plane(P0[-1])
    USap = None
    if Us is not None:
        us = np.array(Us, dtype=np.float64)
        us[np.isnan(us)] = 0.0
        USap = [us]
        for scl in range(1, len(P0)):
            cols, rows = P0[scl].shape[-2:]
            USap.append(pyramid.resize(USap[-1] * p["scl_factor"], rows, cols, "bilinear", out_dtype=np.float64))
        U = dev.to_device(USap[-1].astype(np.float32))
    for scl in range(len(P0) - 1, -1, -1):
        (a0, a1), (b0, b1) = _terms(P0[scl], P1[scl], fstTerm, sndTerm)
        if USap is None:
            U = level.run(a0, a1, U, b0, b1)
        else:
            us64 = torch.from_numpy(np.ascontiguousarray(USap[scl].T)).to(U.device)
            U = level.run(a0, a1, U, b0, b1, Us=us64, as_diff=1.75 * p["scl_factor"] ** scl, u_double=(scl == len(P0) - 1))
        if scl > 0:
            cols, rows = P0[scl - 1].shape[-2:]
            U = _up(U, 1.0 / p["scl_factor"], rows, cols)
    dev.sync_check()
    return dev.to_matlab(U)


SYM_DEFAULTS = dict(alpha=0.035, beta=0.4, omega=1.9, firstLoop=3, secondLoop=4, iter=4, b1=0.25, b2=0.72, scl_factor=0.75, solver=2)


def _disp_sym_planes(Il, Ir, mode, param):
    """The level loop of DispEminND_llin_sym_2D: the two disparities as resident planes [ncols, nrows]; nothing is downloaded."""
    p = dict(SYM_DEFAULTS, **param)
    # no /255 in this driver (:81-82); its coarsest scale stays unsmoothed (:94-98)
    P0, P1 = pyramid.build_dev(_c3(Il), _c3(Ir), p["scl_factor"], 10, pyramid.gaussian(3, 1.0), smooth_last=False)
    level = fl.DispSymLevel(p, mode=mode)
    U0 = _zeros_like_plane(P0[-1])
    U1 = torch.zeros_like(U0)
    for scl in range(len(P0) - 1, -1, -1):
        sr = 2.0 * (1.0 / p["scl_factor"]) ** (-scl)              # srDiff = 2*(1/scl_factor)^-(scl-1), scl 1-based there
        U0, U1 = level.run(P0[scl], P1[scl], U0, U1, sr)
        if scl > 0:
            cols, rows = P0[scl - 1].shape[-2:]
            U0, U1 = _up(U0, 1.0 / p["scl_factor"], rows, cols), _up(U1, 1.0 / p["scl_factor"], rows, cols)
    return U0, U1


def DispEminND_llin_sym_2D(Il, Ir, mode=capi.MODE_EXACT_ORDER, **param):
    """-> U [nrows, ncols, 2] (left-to-right and right-to-left disparity)."""
    U0, U1 = _disp_sym_planes(Il, Ir, mode, param)
    dev.sync_check()
    return np.stack([dev.to_matlab(U0), dev.to_matlab(U1)], axis=2)


def stereo_maps(Il, Ir, tol=1.0, mode=capi.MODE_EXACT_ORDER, fill=False, fill_param=None, **param):
    """DispEminND_llin_sym_2D followed by the left-right check of its two views against each other (device.disp_crosscheck), all on
    the device with one download at the end.  Returns a dict: dense [rows, cols, 2], the driver's two disparities; sparse
    [rows, cols, 2], the same with NaN where a view disagrees with the other by more than tol pixels or looks outside it; mask
    [rows, cols, 2], 1 where kept; stats, two vectors {kept, defined, mean |r|, largest |r|}.  sparse[:, :, 0] is a map as
    DispSegmentationSparse, nanmedfilt2 and sparse_pyramid take it.
    fill=True: each view's sparse map is inpainted on the device (TVinpaint4 with fill_param, that view's image as the guide) and
    comes back under the further key filled [rows, cols, 2]."""
    fp = _inpaint_param("stereo_maps", fill_param or {}) if fill else None
    U0, U1 = _disp_sym_planes(Il, Ir, mode, param)
    U0, U1 = U0.contiguous(), U1.contiguous()
    checked = [dev.disp_crosscheck(a, b, tol=tol, sparse_out=torch.empty_like(a), mask_out=torch.empty_like(a), planes=False)
               for a, b in ((U0, U1), (U1, U0))]
    filled = [_inpaint_planes(c[0], _c3(I), mode, fp)[0] for c, I in zip(checked, (Il, Ir))] if fill else None
    dev.sync_check()
    down = lambda k, src: np.stack([dev.to_matlab(src[0][k]), dev.to_matlab(src[1][k])], axis=2)
    maps = dict(dense=np.stack([dev.to_matlab(U0), dev.to_matlab(U1)], axis=2), sparse=down(0, checked), mask=down(1, checked),
                stats=[c[3].cpu().numpy() for c in checked])
    if fill:
        maps["filled"] = np.stack([dev.to_matlab(filled[0]), dev.to_matlab(filled[1])], axis=2)
    return maps


def _tv(I_in, level_cls, p, G, smooth_last):
    Iin = [dev.to_device(np.asarray(I_in, dtype=np.float32))]
    cols, rows = Iin[0].shape[-2:]
    ds_rows, ds_cols = math.ceil(rows * p["scl"]), math.ceil(cols * p["scl"])
    while True:
        c, r = Iin[-1].shape[-2:]
        nr, nc = int(math.ceil(r * p["scl_factor"])), int(math.ceil(c * p["scl_factor"]))
        Iin.append(dev.pyr_resize(Iin[-1], nr, nc))
        Iin[-2] = dev.pyr_smooth(Iin[-2], G)
        if nr <= ds_rows or nc <= ds_cols:
            if smooth_last:
                Iin[-1] = dev.pyr_smooth(Iin[-1], G)
            break
    level = level_cls(p, mode=p["mode"])
    Iout = Iin[-1]
    for scl in range(len(Iin) - 1, -1, -1):
        Iout = level.run(Iin[scl], Iout)
        if scl > 0:
            c, r = Iin[scl - 1].shape[-2:]
            Iout = dev.pyr_resize(Iout, r, c)
    dev.sync_check()
    return dev.to_matlab(Iout)


def TVdenoise8(I_in, mode=capi.MODE_EXACT_ORDER, **param):
    """TVdenoise8.m; I_in in 0..1.  The coarsest scale is not smoothed: the driver writes that result to a misspelt variable (:72)."""
    p = dict(dict(alpha=500.0, omega=1.75, outer_iter=20, inner_iter=4, solver=2, scl=0.75, scl_factor=0.75), mode=mode, **param)
    return _tv(I_in, fl.TvLevel, p, pyramid.gaussian(5, 1.25), smooth_last=False)


def TVdenoise4(I_in, mode=capi.MODE_EXACT_ORDER, **param):
    p = dict(dict(alpha=5.0, omega=1.75, outer_iter=10, inner_iter=5, solver=2, scl=0.5, scl_factor=0.75), mode=mode, **param)
    return _tv(I_in, fl.Tv4Level, p, pyramid.gaussian(7, 2.0), smooth_last=True)


# ---- the same eight drivers through the C-ABI (what the MEX stubs call): host arrays in, host arrays out --------------------
_TERM = {"NONE": 0, "RGB": 1, "GRAD": 2, "GRADMAG": 3}


def _c_struct(double_fields, int_fields, param):
    """A parameter struct of include/pdeip.h (its doubles, then its ints) filled from `param`; 0, as for a name left out: the driver's default."""
    class P(ctypes.Structure):
        _fields_ = [(k, ctypes.c_double) for k in double_fields] + [(k, ctypes.c_int) for k in int_fields]
    s = P()
    for k, _ in P._fields_:
        setattr(s, k, type(getattr(s, k))(param.get(k, 0) or 0))
    return s


def _c_params(param):   # pdeip_driver_params
    return _c_struct(("alpha", "omega", "gammaS", "b1", "b2", "scl_factor"), ("firstLoop", "secondLoop", "iter", "solver", "scales"), param)


@contextlib.contextmanager
def _ordering(mode):
    """The library's sweep ordering set to `mode` for one C-ABI call, then put back."""
    old = capi.get_mode()
    capi.set_mode(mode)
    try:
        yield
    finally:
        capi.set_mode(old)


def _f_single(a):
    a = np.asarray(a, dtype=np.float32)
    return np.asfortranarray(a if a.ndim == 3 else a[:, :, None])


def _f_double(a):
    return None if a is None else np.asfortranarray(np.asarray(a, dtype=np.float64))


def _ptr(a):
    return None if a is None else a.ctypes.data


def _flow_out(I):
    rows, cols = I.shape[:2]
    return rows, cols, np.zeros((rows, cols), np.float32, order="F"), np.zeros((rows, cols), np.float32, order="F")


def capi_FlowEminND_llin_2D_v10(Iin, channels, fstTerm="rgb", sndTerm="none", mode=capi.MODE_EXACT_ORDER, Us=None, Vs=None, **param):
    """pdeip_flow_nd_llin on MATLAB-shaped numpy arrays: the C++ twin of FlowEminND_llin_2D_v10 above, same bits."""
    I, us, vs, prm = _f_single(Iin), _f_double(Us), _f_double(Vs), _c_params(param)
    rows, cols, U, V = _flow_out(I)
    with _ordering(mode):
        capi.call("pdeip_flow_nd_llin", I.ctypes.data, rows, cols, int(channels), _TERM[fstTerm.upper()], _TERM[sndTerm.upper()], ctypes.addressof(prm),
                  _ptr(us), _ptr(vs), U.ctypes.data, V.ctypes.data)
    return U, V


def capi_DispEminND_llin_2D(Il, Ir, fstTerm="rgb", sndTerm="none", mode=capi.MODE_EXACT_ORDER, Us=None, **param):
    """pdeip_disp_nd_llin on MATLAB-shaped numpy arrays."""
    L, R, us, prm = _f_single(Il), _f_single(Ir), _f_double(Us), _c_params(param)
    rows, cols, C = L.shape
    U = np.zeros((rows, cols), np.float32, order="F")
    with _ordering(mode):
        capi.call("pdeip_disp_nd_llin", L.ctypes.data, R.ctypes.data, rows, cols, C, _TERM[fstTerm.upper()], _TERM[sndTerm.upper()], ctypes.addressof(prm),
                  _ptr(us), U.ctypes.data)
    return U


def _capi_tv(entry, I_in, mode, param):
    I = _f_single(I_in)
    rows, cols, F = I.shape
    out = np.zeros((rows, cols, F), np.float32, order="F")
    prm = _c_struct(("alpha", "omega", "scl", "scl_factor"), ("outer_iter", "inner_iter", "solver"), param)   # pdeip_tv_params
    with _ordering(mode):
        capi.call(entry, I.ctypes.data, rows, cols, F, ctypes.addressof(prm), out.ctypes.data)
    return out if np.asarray(I_in).ndim == 3 else out[:, :, 0]


def capi_TVdenoise8(I_in, mode=capi.MODE_EXACT_ORDER, **param):
    """pdeip_tvdenoise8 on a MATLAB-shaped numpy array: the C++ twin of TVdenoise8 above, same bits."""
    return _capi_tv("pdeip_tvdenoise8", I_in, mode, param)


def capi_TVdenoise4(I_in, mode=capi.MODE_EXACT_ORDER, **param):
    """pdeip_tvdenoise4: the C++ twin of TVdenoise4."""
    return _capi_tv("pdeip_tvdenoise4", I_in, mode, param)


def capi_FlowEminHS_elin_2D_v10(Iin, channels, mode=capi.MODE_EXACT_ORDER, **param):
    """pdeip_flow_hs_elin: the C++ twin of FlowEminHS_elin_2D_v10 above, same bits."""
    I, prm = _f_single(Iin), _c_params(param)
    rows, cols, U, V = _flow_out(I)
    with _ordering(mode):
        capi.call("pdeip_flow_hs_elin", I.ctypes.data, rows, cols, int(channels), ctypes.addressof(prm), U.ctypes.data, V.ctypes.data)
    return U, V


def capi_DispEminND_llin_sym_2D(Il, Ir, mode=capi.MODE_EXACT_ORDER, **param):
    """pdeip_disp_nd_llin_sym: the C++ twin of DispEminND_llin_sym_2D above, same bits; -> U [nrows, ncols, 2]."""
    prm = _c_struct(("alpha", "beta", "omega", "b1", "b2", "scl_factor"), ("firstLoop", "secondLoop", "iter", "solver"), param)   # pdeip_sym_params
    L, R = _f_single(Il), _f_single(Ir)
    rows, cols, C = L.shape
    U = np.zeros((rows, cols, 2), np.float32, order="F")
    with _ordering(mode):
        capi.call("pdeip_disp_nd_llin_sym", L.ctypes.data, R.ctypes.data, rows, cols, C, ctypes.addressof(prm), U.ctypes.data)
    return U


def capi_FlowEminAD_llin_2D_v10(Iin, channels, fstTerm="rgb", sndTerm="none", mode=capi.MODE_EXACT_ORDER, Us=None, Vs=None, quantile=0.0, diffusion="image", **param):
    """pdeip_flow_ad_llin: the C++ twin of FlowEminAD_llin_2D_v10 above, same bits."""
    I, us, vs, prm = _f_single(Iin), _f_double(Us), _f_double(Vs), _c_params(param)
    rows, cols, U, V = _flow_out(I)
    with _ordering(mode):
        capi.call("pdeip_flow_ad_llin", I.ctypes.data, rows, cols, int(channels), _TERM[fstTerm.upper()], _TERM[sndTerm.upper()], ctypes.addressof(prm),
                  float(quantile), int(str(diffusion).lower() == "flow"), _ptr(us), _ptr(vs), U.ctypes.data, V.ctypes.data)
    return U, V


def capi_FlowEminNDFASFMG_elin_2D_v10(Iin, channels, mode=capi.MODE_EXACT_ORDER, **param):
    """pdeip_flow_fas_fmg_elin: the C++ twin of FlowEminNDFASFMG_elin_2D_v10 above, same bits."""
    prm = _c_struct(("alpha", "omega", "b1", "b2", "scl_factor"), ("firstLoop", "iter", "solver", "cycle_index", "scales"), param)   # pdeip_fas_params
    I = _f_single(Iin)
    rows, cols, U, V = _flow_out(I)
    with _ordering(mode):
        capi.call("pdeip_flow_fas_fmg_elin", I.ctypes.data, rows, cols, int(channels), ctypes.addressof(prm), U.ctypes.data, V.ctypes.data)
    return U, V


class _GacParams(__import__("ctypes").Structure):
    _fields_ = [(k, __import__("ctypes").c_double) for k in ("tau", "c", "lambda_", "iter", "smooth")]


_GAC_KEYS = {"tau": "tau", "c": "c", "lambda": "lambda_", "lambda_": "lambda_", "ITER": "iter", "SMOOTH": "smooth"}


def _gac(Iin, PHIin, model, param):
    prm = _GacParams(*([float("nan")] * 5))  # NaN: the driver's default
    for k, v in param.items():
        if k not in _GAC_KEYS or (model == 1 and k == "c"):
            raise TypeError("GAC_v10%s: unknown parameter %r" % ("ab"[model], k))
        setattr(prm, _GAC_KEYS[k], float(v))
    I = np.asfortranarray(np.asarray(Iin, dtype=np.float32))
    P = np.asfortranarray(np.asarray(PHIin, dtype=np.float32))
    rows, cols = I.shape[:2]
    if P.shape != (rows, cols):
        raise ValueError("PHIin is %s but the image is %s" % (P.shape, (rows, cols)))
    out = np.zeros((rows, cols), np.float32, order="F")
    capi.call("pdeip_gac", I.ctypes.data, rows, cols, I.shape[2] if I.ndim == 3 else 1, P.ctypes.data, model,
              ctypes.addressof(prm), out.ctypes.data)
    return out


def GAC_v10a(Iin, PHIin, **param):
    """PHIout = GAC_v10a(Iin, PHIin, ...) (matlab/active_contour/GAC_v10a.m): geodesic active contour with a balloon force, the
    whole run in one pdeip_gac call.  Iin single [rows, cols(, C)] (runme.m divides by 255); param: tau, c, lambda (pass it as
    **{"lambda": v} or lambda_=v; < 0: automatic), ITER, SMOOTH, as the driver names them."""
    return _gac(Iin, PHIin, 0, param)


def GAC_v10b(Iin, PHIin, **param):
    """PHIout = GAC_v10b(Iin, PHIin, ...) (matlab/active_contour/GAC_v10b.m): geodesic active contour with the convection term
    grad(g) . grad(PHI); parameters as GAC_v10a without c."""
    return _gac(Iin, PHIin, 1, param)


def uint8_matlab(x):
    """MATLAB's uint8(x) of a float array: round half away from zero, saturate to 0..255, NaN -> 0.  (numpy's round is half
    to even.)  In double, x + 0.5 is exact for every single x, so floor(x + 0.5) rounds the half away from zero once x >= 0."""
    y = np.asarray(x, dtype=np.float64)
    y = np.clip(np.where(np.isnan(y), 0.0, y), 0.0, 255.0)
    return np.floor(y + 0.5).astype(np.uint8)


def Diffusion4_v10(I_in, as_single=False, **param):
    """Iout = Diffusion4_v10(I_in, ...) (matlab/diffusion/Diffusion4_v10.m): nonlinear (lagged-diffusivity) diffusion, the whole
    run in one pdeip_diffusion4 call.  I_in [rows, cols(, C)] in any numeric type, taken as single(I_in); param: alpha (25),
    outer_iter (5), as the driver names them.  Returns uint8(Iout) by MATLAB's rule, or the single Iout with as_single=True."""
    for k in param:
        if k not in ("alpha", "outer_iter"):
            raise TypeError("Diffusion4_v10: unknown parameter %r" % k)
    prm = dev.Diffusion4Params(float(param.get("alpha", math.nan)), float(param.get("outer_iter", math.nan)))
    I = np.asfortranarray(np.asarray(I_in, dtype=np.float32))
    if I.ndim not in (2, 3):
        raise ValueError("Diffusion4_v10: I_in must be [rows, cols] or [rows, cols, C] (got %s)" % (I.shape,))
    out = np.empty(I.shape, np.float32, order="F")
    capi.call("pdeip_diffusion4", I.ctypes.data, I.shape[0], I.shape[1], I.shape[2] if I.ndim == 3 else 1, ctypes.addressof(prm),
              out.ctypes.data)
    return out if as_single else uint8_matlab(out)


def _image_single(who, I_in):
    I = np.asfortranarray(np.asarray(I_in, dtype=np.float32))
    if I.ndim not in (2, 3):
        raise ValueError("%s: the image must be [rows, cols] or [rows, cols, C] (got %s)" % (who, I.shape))
    return I


def gaussian(I, sigma):
    """G_sigma * I per channel, separable with 'replicate' borders (pdeip_gauss): the smoothing at a chosen scale that runme.m
    loads from a pre-smoothed file, e.g. GAC_v10a(gaussian(I, 2), PHI).  I [rows, cols(, C)] in any numeric type, taken as
    single; returns single."""
    I = _image_single("gaussian", I)
    out = np.empty(I.shape, np.float32, order="F")
    capi.call("pdeip_gauss", I.ctypes.data, I.shape[0], I.shape[1], I.shape[2] if I.ndim == 3 else 1, float(sigma), out.ctypes.data)
    return out


def Diffusion8(I_in, mode="ced", as_single=False, **param):
    """Structure-tensor anisotropic diffusion of I_in [rows, cols(, C)], 0..255 data as Diffusion4_v10 takes it: mode 'ced'
    (coherence-enhancing: smooths along the locally dominant orientation) or 'eed' (edge-enhancing: along edges, not across them).
    The image is uploaded once and filtered by one pdeip_diffusion8_dev call in the library's current ordering.  param: sigma, rho,
    lambda (pass **{"lambda": v} or lambda_=v), alpha, C, tau, iters, inner_iter, omega, solver; defaults in include/pdeip.h.
    Returns uint8(Iout) by MATLAB's rule, or the single Iout with as_single=True."""
    prm = dev.diffusion8_params(mode, "Diffusion8", **param)
    I = _image_single("Diffusion8", I_in)
    t = dev.to_device(I)
    dev.diffusion8(t, prm, t)
    dev.sync_check()
    out = dev.to_matlab(t)
    return out if as_single else uint8_matlab(out)


def capi_Diffusion8(I_in, mode="ced", as_single=False, **param):
    """pdeip_diffusion8 on a MATLAB-shaped numpy array: the host-pointer twin of Diffusion8 above, same bits."""
    prm = dev.diffusion8_params(mode, "capi_Diffusion8", **param)
    I = _image_single("capi_Diffusion8", I_in)
    out = np.empty(I.shape, np.float32, order="F")
    capi.call("pdeip_diffusion8", I.ctypes.data, I.shape[0], I.shape[1], I.shape[2] if I.ndim == 3 else 1, ctypes.addressof(prm),
              out.ctypes.data)
    return out if as_single else uint8_matlab(out)


def SurfaceEquation(A, B, M_in, err_thr, min_set_size, iter, seed=None, sets=None):
    """[M_out, Err] = SurfaceEquation(A, B, M_in, err_thr, min_set_size, iter) (mex/source/SurfaceEquation.c): the RANSAC fit of a
    first- ([X Y 1]) or second-order ([X^2 Y^2 XY X Y 1]) polynomial surface in one pdeip_surface_equation call.  Arguments in any
    numeric type, taken as single; M_in None or empty: none.  seed / sets choose the samples (include/pdeip.h); without either a
    seed is drawn from the clock once and advanced per call.  Returns M_out [ncoef, 1] and Err [ndata, 1] as the gateway does."""
    from . import mex_api

    A = np.asarray(A, dtype=np.float32)
    B = np.asarray(B, dtype=np.float32).reshape(-1)
    if A.ndim != 2 or A.shape[0] != B.size:
        raise ValueError("SurfaceEquation: A is %s but B has %d elements" % (A.shape, B.size))
    if M_in is not None and np.size(M_in) == 0:
        M_in = None
    if M_in is not None and np.size(M_in) != A.shape[1]:
        raise ValueError("SurfaceEquation: M_in must have as many elements as A has columns")
    M, err, _, _ = mex_api.surface_equation(A, B, M_in, float(np.float32(err_thr)), float(np.float32(min_set_size)), int(iter), seed, sets)
    return np.asfortranarray(M.reshape(-1, 1)), np.asfortranarray(err.reshape(-1, 1))


def _planes3(PHI):
    P = np.asarray(PHI, dtype=np.float32)
    if P.ndim == 2:
        P = P[:, :, None]
    if P.ndim != 3 or P.shape[2] < 1:
        raise ValueError("PHI must be [rows, cols, segments] with at least one segment (got %s)" % (P.shape,))
    return np.asfortranarray(P)


def regionCompetition(D, PHI, polyorder, sigmaLim, ransac_cset, iterations, srem_thr, competition="inverse", sparse=False, seed=0,
                      scl_factor=0.7, rc_scl=0.4, **param):
    """[PHIout SParam] = regionCompetition(D, pyramid, polyorder, sigmaLim, ransac_cset, iterations, srem_thr, PHIin, competition)
    of matlab/segmentation/DispSegmentation.m (sparse=True: DispSegmentationSparse.m's constants) in one pdeip_region_competition
    call: the D pyramid (scl_factor, rc_scl as the drivers' param struct names them), the visits down and up, every iteration
    resident.  param overrides single constants (c0, c1, dh_floor, err_thr, gamma_coef, dist_cap, nan_fill).  Returns (PHI [rows,
    cols, S_out], SParam [ncoef, S_out], kept: the 0-based input index of each surviving segment).
    The sparse driver's own function, nanmedfilt2 pyramid included, is regionCompetitionSparse."""
    return _region_competition("pdeip_region_competition", dev.SegParams.make(sparse=sparse, **param), D, PHI, polyorder, sigmaLim, ransac_cset,
                               iterations, srem_thr, competition, seed, scl_factor, rc_scl)


def regionCompetitionSparse(D, PHI, polyorder, sigmaLim, ransac_cset, iterations, srem_thr, competition="inverse", seed=0, scl_factor=0.75,
                            rc_scl=0.55, **param):
    """regionCompetition() of matlab/segmentation/DispSegmentationSparse.m in one pdeip_region_competition_sparse call: D is the raw
    map with its NaNs, its pyramid is the sparse one (sparse_pyramid), the constants are the sparse driver's unless param overrides
    one.  Arguments and result as regionCompetition."""
    return _region_competition("pdeip_region_competition_sparse", dev.SegParams.make(**param), D, PHI, polyorder, sigmaLim, ransac_cset,
                               iterations, srem_thr, competition, seed, scl_factor, rc_scl)


def _region_competition(entry, prm, D, PHI, polyorder, sigmaLim, ransac_cset, iterations, srem_thr, competition, seed, scl_factor, rc_scl):
    Dm = np.asfortranarray(np.asarray(D, dtype=np.float32))
    P = _planes3(PHI)
    rows, cols, S = P.shape
    if Dm.shape != (rows, cols):
        raise ValueError("regionCompetition: D is %s but PHI is %s" % (Dm.shape, P.shape))
    ncoef = 6 if polyorder == 2 else 3
    out = np.zeros(P.shape, np.float32, order="F")
    surf = np.zeros((ncoef, S), np.float32, order="F")
    kept = (ctypes.c_int * S)()
    s_out = ctypes.c_int(0)
    capi.call(entry, Dm.ctypes.data, P.ctypes.data, rows, cols, S, int(polyorder), dev._strategy(competition),
              float(sigmaLim), float(ransac_cset), int(iterations), float(srem_thr), float(scl_factor), float(rc_scl),
              ctypes.c_ulonglong(int(seed) & ((1 << 64) - 1)), ctypes.addressof(prm), ctypes.addressof(s_out), out.ctypes.data,
              surf.ctypes.data, ctypes.addressof(kept))
    n = s_out.value
    return np.asfortranarray(out[:, :, :n]), np.asfortranarray(surf[:, :n]), [int(k) for k in kept[:n]]


def segments_numbered(PHI):
    """The numbered segment map the drivers return (DispSegmentation.m:190-198): s where only segment s (1-based) has PHI > 0, 0
    where none or several have; int32 [rows, cols], one pdeip_seg_label call."""
    P = _planes3(PHI)
    rows, cols, S = P.shape
    out = np.zeros((rows, cols), np.int32, order="F")
    capi.call("pdeip_seg_label", P.ctypes.data, rows, cols, S, out.ctypes.data)
    return out


def bwlabel(BW, conn=8):
    """[L, num] = bwlabel(BW, conn) with MATLAB's numbering (components 1..num in the order of their first pixel in column-major
    order, 0 for background), one pdeip_bwlabel call.  BW [rows, cols]: a logical array, or numbers of which the positive ones are
    foreground (the drivers call bwlabel(PHI > 0)).  Returns (L float64 [rows, cols] as MATLAB's is, num)."""
    B = np.asarray(BW)
    if B.ndim != 2:
        raise ValueError("bwlabel: BW must be two-dimensional (got %s)" % (B.shape,))
    A = np.asfortranarray((B > 0).astype(np.float32))
    rows, cols = A.shape
    L = np.zeros((rows, cols), np.int32, order="F")
    num = ctypes.c_int(0)
    capi.call("pdeip_bwlabel", A.ctypes.data, rows, cols, int(conn), L.ctypes.data, ctypes.addressof(num), None, 0)
    return np.asfortranarray(L.astype(np.float64)), num.value


class _SeedsParams(ctypes.Structure):
    """pdeip_seeds_params: NaN keeps the dense driver's value."""
    _fields_ = [(k, ctypes.c_double) for k in ("dist_cap", "nan_fill", "mincov_gate")]


class _SeedsTrace(ctypes.Structure):
    """pdeip_seeds_trace."""
    _fields_ = [("counts", ctypes.c_void_p), ("counts_cap", ctypes.c_int), ("n_counts", ctypes.c_int), ("largest", ctypes.c_void_p),
                ("n_largest", ctypes.c_int)]


class _DispSegParams(ctypes.Structure):
    """pdeip_dispseg_params: NaN / 0 keeps the .m's default."""
    _fields_ = [(k, ctypes.c_double) for k in ("srem_thr", "scl_factor", "gen_scl", "rc_scl", "ransac_min_cset", "ransac_max_cset")] + \
               [(k, ctypes.c_int) for k in ("polyorder", "seeds", "ransac_cset_cycles")]


def generateSeeds(D, polyorder, sigmaLim, cset_vect, iterations, AA=None, seeds=15, sparse=False, seed=0, scl_factor=0.7, pyr_scl=0.2,
                  fit_counter=0, trace=None, **param):
    """[PHIout SParam] = generateSeeds(D, pyramid, polyorder, sigmaLim, ransac_cset_vect, iterations, srem_thr, AAin, seeds) of
    matlab/segmentation/DispSegmentation.m (sparse=True: DispSegmentationSparse.m's constants dist_cap 100, nan_fill 1000,
    mincov_gate 0.5) in one pdeip_generate_seeds call; the pyramid is given by scl_factor and pyr_scl (the drivers' gen_scl or
    rc_scl).  param overrides single constants.  trace: a dict that receives counts (every count read back), largest (the v = K
    largest-component planes [rK, cK, n]) and fit_counter.  Returns (PHI [rows, cols, S_out], SParam [ncoef, S_out]).
    The sparse driver's own function, nanmedfilt2 pyramid and starting gamma included, is generateSeedsSparse."""
    vals = dict(dist_cap=100.0, nan_fill=1000.0, mincov_gate=0.5) if sparse else {}
    return _generate_seeds("pdeip_generate_seeds", vals, D, polyorder, sigmaLim, cset_vect, iterations, AA, seeds, seed, scl_factor, pyr_scl,
                           fit_counter, trace, param)


def generateSeedsSparse(D, polyorder, sigmaLim, cset_vect, iterations, AA=None, seeds=15, seed=0, scl_factor=0.75, pyr_scl=0.55, fit_counter=0,
                        trace=None, **param):
    """generateSeeds() of matlab/segmentation/DispSegmentationSparse.m in one pdeip_generate_seeds_sparse call: D is the raw map with
    its NaNs, its pyramid is the sparse one (sparse_pyramid), gamma starts at 0.005, the constants are the sparse driver's unless
    param overrides one.  Arguments and result as generateSeeds."""
    return _generate_seeds("pdeip_generate_seeds_sparse", {}, D, polyorder, sigmaLim, cset_vect, iterations, AA, seeds, seed, scl_factor,
                           pyr_scl, fit_counter, trace, param)


def _generate_seeds(entry, vals, D, polyorder, sigmaLim, cset_vect, iterations, AA, seeds, seed, scl_factor, pyr_scl, fit_counter, trace, param):
    for k, v in param.items():
        if k not in dict(_SeedsParams._fields_):
            raise TypeError("unknown generateSeeds parameter %r" % k)
        vals[k] = float(v)
    prm = _SeedsParams(*[vals.get(k, float("nan")) for k, _ in _SeedsParams._fields_])
    Dm = np.asfortranarray(np.asarray(D, dtype=np.float32))
    if Dm.ndim != 2:
        raise ValueError("generateSeeds: D must be two-dimensional (got %s)" % (Dm.shape,))
    rows, cols = Dm.shape
    Am = None
    if AA is not None:
        Am = np.asfortranarray(np.asarray(AA, dtype=np.float32))
        if Am.shape != Dm.shape:
            raise ValueError("generateSeeds: AA is %s but D is %s" % (Am.shape, Dm.shape))
    cs = np.ascontiguousarray(np.asarray(cset_vect, dtype=np.float64).reshape(-1))
    seeds, iterations = int(seeds), int(iterations)
    ncoef = 6 if polyorder == 2 else 3
    n = max(seeds, 1)
    out = np.zeros((rows, cols, n), np.float32, order="F")
    surf = np.zeros((ncoef, n), np.float32, order="F")
    s_out = ctypes.c_int(0)
    fit = ctypes.c_ulonglong(int(fit_counter) & ((1 << 64) - 1))
    tr, counts, largest = None, None, None
    if trace is not None:
        cap = n * (max(iterations, 0) + 1) * 64
        counts = np.zeros(cap, np.int32)
        largest = np.zeros(rows * cols * n, np.float32)  # no scale is larger than the first
        tr = _SeedsTrace(counts.ctypes.data, cap, 0, largest.ctypes.data, 0)
    capi.call(entry, Dm.ctypes.data, None if Am is None else Am.ctypes.data, rows, cols, int(polyorder), float(sigmaLim),
              cs.ctypes.data, int(cs.size), iterations, seeds, float(scl_factor), float(pyr_scl),
              ctypes.c_ulonglong(int(seed) & ((1 << 64) - 1)), ctypes.addressof(fit), ctypes.addressof(prm),
              None if tr is None else ctypes.addressof(tr), ctypes.addressof(s_out), out.ctypes.data, surf.ctypes.data)
    if trace is not None:
        trace["counts"] = [int(c) for c in counts[:min(tr.n_counts, tr.counts_cap)]]
        trace["n_counts"] = tr.n_counts
        trace["largest"] = largest[:0] if tr.n_largest == 0 else largest
        trace["n_largest"] = tr.n_largest
        trace["fit_counter"] = int(fit.value)
    k = s_out.value
    return np.asfortranarray(out[:, :, :k]), np.asfortranarray(surf[:, :k])


def DispSegmentation(Din, seed=0, PHI=None, AA=None, **param):
    """[PHI SEG SParam] = DispSegmentation(Din, param) of matlab/segmentation/DispSegmentation.m in one pdeip_disp_segmentation
    call.  param: the .m's fields srem_thr, polyorder, seeds, scl_factor, gen_scl, rc_scl, ransac_min_cset, ransac_max_cset,
    ransac_cset_cycles (defaults as there); PHI (param.PHI) and AA (param.AA) as keywords.  Returns (PHI [rows, cols, S], SEG int32
    [rows, cols], SParam [ncoef, S]); with no segment left: S = 0 and SEG all zero."""
    return _disp_segmentation("pdeip_disp_segmentation", "DispSegmentation", 1, Din, seed, PHI, AA, param)


def DispSegmentationSparse(Din, seed=0, PHI=None, AA=None, **param):
    """[PHI SEG SParam] = DispSegmentationSparse(Din, param) of matlab/segmentation/DispSegmentationSparse.m in one
    pdeip_disp_segmentation_sparse call: Din's NaNs mean "no estimate" and stay in place.  param, PHI, AA and the result as
    DispSegmentation, the defaults as the sparse .m has them (polyorder 2, scl_factor 0.75, gen_scl 0.55, rc_scl 0.55)."""
    return _disp_segmentation("pdeip_disp_segmentation_sparse", "DispSegmentationSparse", 2, Din, seed, PHI, AA, param)


def _disp_segmentation(entry, name, default_order, Din, seed, PHI, AA, param):
    names = dict(_DispSegParams._fields_)
    for k in param:
        if k not in names:
            raise TypeError("unknown %s parameter %r" % (name, k))
    prm = _DispSegParams(*[(float(param.get(k, float("nan"))) if t is ctypes.c_double else int(param.get(k, 0))) for k, t in _DispSegParams._fields_])
    Dm = np.asfortranarray(np.asarray(Din, dtype=np.float32))
    if Dm.ndim != 2:
        raise ValueError(name + ": Din must be two-dimensional (got %s)" % (Dm.shape,))
    rows, cols = Dm.shape
    Pm, S_in = None, 0
    if PHI is not None:
        Pm = _planes3(PHI)
        S_in = Pm.shape[2]
        if Pm.shape[:2] != Dm.shape:
            raise ValueError("%s: PHI is %s but Din is %s" % (name, Pm.shape, Dm.shape))
    Am = None
    if AA is not None:
        Am = np.asfortranarray(np.asarray(AA, dtype=np.float32))
        if Am.shape != Dm.shape:
            raise ValueError("%s: AA is %s but Din is %s" % (name, Am.shape, Dm.shape))
    polyorder = int(param.get("polyorder", 0)) or default_order  # 0 keeps the .m's default, as in the C call
    n_seeds = int(param.get("seeds", 0)) or 15
    cap = max(S_in + 1 if Pm is not None else 2 * n_seeds, 1)
    ncoef = 6 if polyorder == 2 else 3
    out = np.zeros((rows, cols, cap), np.float32, order="F")
    surf = np.zeros((ncoef, cap), np.float32, order="F")
    SEG = np.zeros((rows, cols), np.int32, order="F")
    s_out = ctypes.c_int(0)
    capi.call(entry, Dm.ctypes.data, rows, cols, None if Pm is None else Pm.ctypes.data, S_in,
              None if Am is None else Am.ctypes.data, ctypes.addressof(prm), ctypes.c_ulonglong(int(seed) & ((1 << 64) - 1)),
              ctypes.addressof(s_out), out.ctypes.data, SEG.ctypes.data, surf.ctypes.data)
    k = s_out.value
    return np.asfortranarray(out[:, :, :k]), SEG, np.asfortranarray(surf[:, :k])


def nanmedfilt2(D):
    """D = nanmedfilt2(D) of matlab/segmentation/DispSegmentationSparse.m:679-685 (colfilt(D, [3 3], 'sliding', @nanmedian)) in one
    pdeip_nanmedfilt2 call: the NaN-ignoring median of each 3x3 window, the positions outside the plane holding the value 0; even
    counts give the mean of the two middle values, a window of nine NaNs gives NaN.  D [rows, cols] or [rows, cols, F]."""
    Dm = np.asfortranarray(np.asarray(D, dtype=np.float32))
    if Dm.ndim not in (2, 3):
        raise ValueError("nanmedfilt2: D must be [rows, cols] or [rows, cols, F] (got %s)" % (Dm.shape,))
    out = np.empty(Dm.shape, np.float32, order="F")
    capi.call("pdeip_nanmedfilt2", Dm.ctypes.data, Dm.shape[0], Dm.shape[1], Dm.shape[2] if Dm.ndim == 3 else 1, out.ctypes.data)
    return out


def sparse_pyramid(D, scl_factor=0.75, pyr_scl=0.55):
    """The D pyramid of DispSegmentationSparse.m:63-79 in one pdeip_sparse_pyramid call: P[0] = nanmedfilt2(D), P[k+1] =
    nanmedfilt2(imresize(nanmedfilt2(P[k]), scl_factor)), down to the last scale with both sides >= pyr_scl x the original.
    Returns the list of the scales' arrays."""
    Dm = np.asfortranarray(np.asarray(D, dtype=np.float32))
    if Dm.ndim != 2:
        raise ValueError("sparse_pyramid: D must be two-dimensional (got %s)" % (Dm.shape,))
    rows, cols = Dm.shape
    cap = 64
    K = ctypes.c_int(0)
    sizes = (ctypes.c_int * (2 * cap))()
    capi.call("pdeip_sparse_pyramid", Dm.ctypes.data, rows, cols, float(scl_factor), float(pyr_scl), cap, ctypes.addressof(K),
              ctypes.addressof(sizes), None)
    shapes = [(sizes[2 * k], sizes[2 * k + 1]) for k in range(K.value)]
    out = np.empty(sum(r * c for r, c in shapes), np.float32)
    capi.call("pdeip_sparse_pyramid", Dm.ctypes.data, rows, cols, float(scl_factor), float(pyr_scl), cap, ctypes.addressof(K),
              ctypes.addressof(sizes), out.ctypes.data)
    planes, at = [], 0
    for r, c in shapes:
        planes.append(np.asfortranarray(out[at:at + r * c].reshape(c, r).T))
        at += r * c
    return planes


def flow2color(flow, uint8=False, return_max=False, **param):
    """img = flow2color(flow, 'maxvalue', m, 'border', b) (matlab/optical_flow/flow2color.m) in one pdeip_flow2color call: hue
    codes the direction, intensity the magnitude over maxvalue (default: the field's largest magnitude), invalid pixels are white;
    border > 0 adds the direction frame, the flow's picture pasted at the .m's offset border - 1.  flow [rows, cols, 2] in any numeric
    type, taken as single(flow).  Returns the single picture [rows + 2 b, cols + 2 b, 3], or with uint8=True uint8(round(255 img)) as
    [rows + 2 b, cols + 2 b, 3] in C order; with return_max=True, (img, maxvalue), the maximum the .m displays."""
    for k in param:
        if k not in ("maxvalue", "border"):
            raise TypeError("flow2color: unknown parameter %r" % k)
    F = np.asarray(flow, dtype=np.float32)
    if F.ndim != 3 or F.shape[2] != 2:
        raise ValueError("flow2color: flow must be [rows, cols, 2] (got %s)" % (F.shape,))
    maxvalue, border = param.get("maxvalue"), param.get("border", 0)
    if maxvalue is not None and np.size(maxvalue) == 0:
        maxvalue = None  # the .m's empty default
    if border != int(border) or border < 0:
        raise ValueError("flow2color: border must be a non-negative integer (got %r)" % (border,))
    border = int(border)
    U, V = np.asfortranarray(F[:, :, 0]), np.asfortranarray(F[:, :, 1])
    rows, cols = U.shape
    brows, bcols = rows + 2 * border, cols + 2 * border
    img = np.empty((brows, bcols, 3), np.uint8) if uint8 else np.empty((brows, bcols, 3), np.float32, order="F")
    used = ctypes.c_double(0.0)
    capi.call("pdeip_flow2color", U.ctypes.data, V.ctypes.data, rows, cols, math.nan if maxvalue is None else float(maxvalue), border,
              None if uint8 else img.ctypes.data, img.ctypes.data if uint8 else None, ctypes.addressof(used))
    return (img, used.value) if return_max else img


def flow_errors(U, V, Utrue, Vtrue, mask=None):
    """The flow (U, V) against the ground truth in one pdeip_flow_errors call.  A pixel counts when the four values are finite and
    mask (nonzero = counts; None: every pixel) allows it.  Returns a dict: epe and ang, the endpoint and Barron's angular error
    (degrees) as single planes with NaN where a pixel does not count; count, mean_epe, mean_ang, max_epe."""
    planes = [np.asfortranarray(np.asarray(a, dtype=np.float32)) for a in (U, V, Utrue, Vtrue)]
    if planes[0].ndim != 2 or any(p.shape != planes[0].shape for p in planes):
        raise ValueError("flow_errors: U, V, Utrue and Vtrue must be [rows, cols] arrays of one shape")
    m = None
    if mask is not None:
        m = np.asfortranarray(np.asarray(mask, dtype=np.float32))
        if m.shape != planes[0].shape:
            raise ValueError("flow_errors: mask must have the flow's shape")
    rows, cols = planes[0].shape
    epe, ang = np.empty((rows, cols), np.float32, order="F"), np.empty((rows, cols), np.float32, order="F")
    stats = (ctypes.c_double * 4)()
    capi.call("pdeip_flow_errors", *[p.ctypes.data for p in planes], None if m is None else m.ctypes.data, rows, cols, epe.ctypes.data,
              ang.ctypes.data, ctypes.addressof(stats))
    return dict(epe=epe, ang=ang, count=int(stats[0]), mean_epe=stats[1], mean_ang=stats[2], max_epe=stats[3])


def _same_planes(who, names, arrays):
    planes = [np.asfortranarray(np.asarray(a, dtype=np.float32)) for a in arrays]
    if planes[0].ndim != 2 or any(p.shape != planes[0].shape for p in planes):
        raise ValueError("%s: %s must be [rows, cols] arrays of one shape" % (who, names))
    return planes


def _threshold(who, name, v):
    v = float(v)
    if not v >= 0.0:
        raise ValueError("%s: %s must be >= 0 and not NaN (got %r)" % (who, name, v))
    return v


def disp_crosscheck(D0, D1, tol=1.0):
    """The left-right check of the disparity D0 against the other view's D1 in one pdeip_disp_crosscheck call (include/pdeip.h): a
    pixel is kept when D1, sampled linearly at x + D0, cancels D0 to within tol pixels.  Returns a dict: sparse (D0 where kept, NaN
    elsewhere), mask (1 / 0), diff (D0 + the sampled D1, NaN where the sample is undefined) as single planes; kept, defined, mean, max."""
    d0, d1 = _same_planes("disp_crosscheck", "D0 and D1", (D0, D1))
    tol = _threshold("disp_crosscheck", "tol", tol)
    rows, cols = d0.shape
    sparse, mask, diff = (np.empty((rows, cols), np.float32, order="F") for _ in range(3))
    stats = (ctypes.c_double * 4)()
    capi.call("pdeip_disp_crosscheck", d0.ctypes.data, d1.ctypes.data, rows, cols, tol, sparse.ctypes.data, mask.ctypes.data,
              diff.ctypes.data, ctypes.addressof(stats))
    return dict(sparse=sparse, mask=mask, diff=diff, kept=int(stats[0]), defined=int(stats[1]), mean=stats[2], max=stats[3])


def flow_crosscheck(Uf, Vf, Ub, Vb, a=0.01, b=0.5):
    """The forward-backward check of the flow (Uf, Vf) of frame 0 -> 1 against (Ub, Vb) of frame 1 -> 0 in one pdeip_flow_crosscheck
    call: a pixel is kept when |f + b(x + f)|^2 <= a (|f|^2 + |b|^2) + b (Sundaram, Brox, Keutzer 2010).  Returns a dict: mask (1 / 0)
    and err (|f + b(x + f)|, NaN where the sample is undefined) as single planes; kept, defined, mean, max."""
    planes = _same_planes("flow_crosscheck", "Uf, Vf, Ub and Vb", (Uf, Vf, Ub, Vb))
    a, b = _threshold("flow_crosscheck", "a", a), _threshold("flow_crosscheck", "b", b)
    rows, cols = planes[0].shape
    mask, err = np.empty((rows, cols), np.float32, order="F"), np.empty((rows, cols), np.float32, order="F")
    stats = (ctypes.c_double * 4)()
    capi.call("pdeip_flow_crosscheck", *[p.ctypes.data for p in planes], rows, cols, a, b, mask.ctypes.data, err.ctypes.data,
              ctypes.addressof(stats))
    return dict(mask=mask, err=err, kept=int(stats[0]), defined=int(stats[1]), mean=stats[2], max=stats[3])


# ---- hole filling: a sparse map (NaN = no estimate) made dense by TV inpainting (include/pdeip.h; this library's own driver) ----
INPAINT_DEFAULTS = dict(alpha=5.0, omega=1.75, outer_iter=10, inner_iter=5, solver=2, scl_factor=0.75, min_size=16, cover=0.25,
                        guide_scale=20.0, keep=1)


def _inpaint_param(who, param):
    """The defaults filled in as pdeip_tv_inpaint4 fills them (a value <= 0 or NaN keeps its default; keep: < 0), and its refusals."""
    unknown = set(param) - set(INPAINT_DEFAULTS)
    if unknown:
        raise ValueError("%s: unknown parameter %s" % (who, sorted(unknown)))
    p = dict(INPAINT_DEFAULTS)
    for k, v in param.items():
        if k == "keep":
            p[k] = 1 if int(v) < 0 else int(int(v) != 0)
        elif v > 0:
            p[k] = type(INPAINT_DEFAULTS[k])(v)
    if p["solver"] not in (1, 2):
        raise ValueError("%s: unknown solver %d (1 point SOR, 2 line relaxation)" % (who, p["solver"]))
    if not p["scl_factor"] < 1.0:
        raise ValueError("%s: scl_factor must be below 1 (got %r)" % (who, p["scl_factor"]))
    if not p["cover"] <= 1.0:
        raise ValueError("%s: cover must not be above 1 (got %r)" % (who, p["cover"]))
    return p


def _inpaint_planes(D, guide, mode, p, want_filled=False):
    """The level loop of pdeip_tv_inpaint4_dev composed from the stage calls, on resident planes: D [(F,) ncols, nrows] with NaN
    holes, guide [(C,) ncols, nrows] or None.  Returns (out, filled or None); nothing is downloaded."""
    Ds, Gs = [D], [guide]
    floor = max(int(p["min_size"]), 3)
    while True:
        c, r = Ds[-1].shape[-2:]
        nr, nc = int(math.ceil(r * p["scl_factor"])), int(math.ceil(c * p["scl_factor"]))
        if min(nr, nc) < floor or (nr == r and nc == c):
            break
        Ds.append(dev.nan_resize(Ds[-1], nr, nc, p["cover"]))
        Gs.append(None if guide is None else dev.pyr_resize(Gs[-1], nr, nc))
    level = fl.Inpaint4Level(p, mode=mode)
    X = dev.inpaint_meanfill(Ds[-1])
    for scl in range(len(Ds) - 1, -1, -1):
        X = level.run(Ds[scl], X, Gs[scl])
        if scl > 0:
            c, r = Ds[scl - 1].shape[-2:]
            X = dev.pyr_resize(X, r, c)
    filled = torch.empty_like(D) if want_filled else None
    if p["keep"]:
        return dev.inpaint_merge(X, D, filled_out=filled), filled
    if want_filled:
        dev.inpaint_merge(X, D, filled_out=filled)
    return X, filled


def _inpaint_inputs(who, D, guide):
    d = np.asarray(D, dtype=np.float32)
    if d.ndim not in (2, 3):
        raise ValueError("%s: D must be [rows, cols] or [rows, cols, frames]" % who)
    g = None if guide is None else np.asarray(guide, dtype=np.float32)
    if g is not None and (g.ndim not in (2, 3) or g.shape[:2] != d.shape[:2]):
        raise ValueError("%s: the guide must be [rows, cols(, channels)] on D's frame" % who)
    return d, g


def TVinpaint4(D, guide=None, mode=capi.MODE_EXACT_ORDER, return_filled=False, **param):
    """Fill the holes (NaN) of the sparse map D [rows, cols(, frames)] by total-variation inpainting: PDEsolver4 with NaN TRACE on
    the holes and TVdenoise4's lagged-diffusivity weights, coarse to fine over a NaN-aware pyramid.  guide [rows, cols(, channels)]:
    an image whose edges (times guide_scale) join the weights, so that a filled region ends where the image says it does.  A flow is
    filled by passing cat(3, U, V).  param: alpha 5, omega 1.75, outer_iter 10, inner_iter 5, solver 2, scl_factor 0.75, min_size 16,
    cover 0.25, guide_scale 20, keep 1 (known pixels come back with their own bits).  Returns the dense map, with return_filled also
    the plane that is 1 on the former holes."""
    p = _inpaint_param("TVinpaint4", param)
    d, g = _inpaint_inputs("TVinpaint4", D, guide)
    out, filled = _inpaint_planes(dev.to_device(d), None if g is None else _c3(g), mode, p, want_filled=return_filled)
    dev.sync_check()
    return (dev.to_matlab(out), dev.to_matlab(filled)) if return_filled else dev.to_matlab(out)


def capi_TVinpaint4(D, guide=None, mode=capi.MODE_EXACT_ORDER, return_filled=False, **param):
    """pdeip_tv_inpaint4 on MATLAB-shaped numpy arrays: the C++ twin of TVinpaint4 above, same bits."""
    d, g = _inpaint_inputs("capi_TVinpaint4", D, guide)
    d3 = _f_single(d)
    rows, cols, F = d3.shape
    g3 = None if g is None else _f_single(g)
    out = np.zeros((rows, cols, F), np.float32, order="F")
    filled = np.zeros((rows, cols, F), np.float32, order="F") if return_filled else None
    prm = dev.InpaintParams.make(**param)
    with _ordering(mode):
        capi.call("pdeip_tv_inpaint4", d3.ctypes.data, rows, cols, F, _ptr(g3), 0 if g3 is None else g3.shape[2],
                  ctypes.addressof(prm), out.ctypes.data, _ptr(filled))
    shape = (lambda a: a if d.ndim == 3 else a[:, :, 0])
    return (shape(out), shape(filled)) if return_filled else shape(out)


# ---- frame interpolation: the picture between two frames, from a computed flow (include/pdeip.h; this library's own driver) ----
def _interp_param(who, param):
    """(mode, InterpParams) of a driver's keyword parameters: mode, a, b, use_costs and TVinpaint4's for the hole filling; with
    fill_with="nearest" (and its max_dist) the nearest-source fill, which takes none of TVinpaint4's."""
    param = dict(param)
    mode = param.pop("mode", capi.MODE_EXACT_ORDER)
    fill_with = param.pop("fill_with", "tv")
    if fill_with not in ("tv", "nearest"):
        raise ValueError("%s: fill_with must be 'tv' or 'nearest' (got %r)" % (who, fill_with))
    nearest = {}
    if fill_with == "nearest":
        nearest = dict(fill_with="nearest", max_dist=int(param.pop("max_dist", 0)))
    fill = {k: param.pop(k) for k in list(param) if k in INPAINT_DEFAULTS}
    unknown = set(param) - {"a", "b", "use_costs"}
    if unknown:
        raise ValueError("%s: unknown parameter %s" % (who, sorted(unknown)))
    if nearest and fill:
        raise ValueError("%s: fill_with='nearest' takes no TV inpainting parameters (got %s)" % (who, sorted(fill)))
    _inpaint_param(who, fill)
    for k in ("a", "b"):
        if k in param:
            param[k] = _threshold(who, k, param[k])
    return mode, dict(param, **fill, **nearest)


def _time(who, t):
    t = float(t)
    if not 0.0 < t < 1.0:
        raise ValueError("%s: t must lie strictly between 0 and 1 (got %r)" % (who, t))
    return t


def flow_interpolate(I0, I1, U, V, Ub=None, Vb=None, t=0.5, return_flow=False, return_source=False, **param):
    """The frame at time t between I0 and I1 [rows, cols(, channels)] from the flow (U, V) of frame 0 -> 1, in one
    pdeip_flow_interpolate call (include/pdeip.h): the flow is carried forward to t (the most photo-consistent source wins a
    pixel), its holes are filled by TV inpainting, and both frames are sampled along it and blended.  With the backward flow
    (Ub, Vb) of frame 1 -> 0 the two forward-backward checks decide at an occlusion which frame alone is shown.  param: mode, a 0.01,
    b 0.5, use_costs 1 and TVinpaint4's; fill_with="nearest" (default "tv") fills the holes with the nearest source's flow instead
    (pdeip_flow_interpolate_nearest; max_dist > 0: only that far, the rest becomes 0) and then refuses TVinpaint4's parameters.
    Returns It, with return_flow also the filled flow at t as [rows, cols, 2], with return_source also the plane 0 neither / 1 frame 0
    / 2 frame 1 / 3 both."""
    who = "flow_interpolate"
    mode, prm_kw = _interp_param(who, param)
    t = _time(who, t)
    if (Ub is None) != (Vb is None):
        raise ValueError("%s: Ub and Vb must both be given or both be None" % who)
    i0, i1 = np.asarray(I0, dtype=np.float32), np.asarray(I1, dtype=np.float32)
    if i0.ndim not in (2, 3) or i0.shape != i1.shape:
        raise ValueError("%s: I0 and I1 must be [rows, cols(, channels)] arrays of one shape" % who)
    names = "U, V" + (", Ub and Vb" if Ub is not None else "")
    planes = _same_planes(who, names, (U, V) + ((Ub, Vb) if Ub is not None else ()))
    if planes[0].shape != i0.shape[:2]:
        raise ValueError("%s: the flow is %s but the frames are %s" % (who, planes[0].shape, i0.shape[:2]))
    f0, f1 = _f_single(i0), _f_single(i1)
    rows, cols, C = f0.shape
    It = np.zeros((rows, cols, C), np.float32, order="F")
    Ut, Vt = ((np.zeros((rows, cols), np.float32, order="F") for _ in range(2)) if return_flow else (None, None))
    src = np.zeros((rows, cols), np.float32, order="F") if return_source else None
    nearest = prm_kw.pop("fill_with", "tv") == "nearest"
    max_dist = prm_kw.pop("max_dist", 0)
    prm = dev.InterpParams.make(**prm_kw)
    head = (f0.ctypes.data, f1.ctypes.data, C, planes[0].ctypes.data, planes[1].ctypes.data, _ptr(planes[2]) if Ub is not None else None,
            _ptr(planes[3]) if Ub is not None else None, rows, cols, t, ctypes.addressof(prm))
    tail = (It.ctypes.data, _ptr(Ut), _ptr(Vt), _ptr(src))
    if nearest:
        capi.call("pdeip_flow_interpolate_nearest", *head, max_dist, *tail)
    else:
        with _ordering(mode):
            capi.call("pdeip_flow_interpolate", *head, *tail)
    out = (It if i0.ndim == 3 else It[:, :, 0],)
    if return_flow:
        out += (np.stack([Ut, Vt], axis=2),)
    if return_source:
        out += (src,)
    return out[0] if len(out) == 1 else out


def interpolate_frames(Iin, channels, t=(0.5,), mode=capi.MODE_EXACT_ORDER, fstTerm="rgb", sndTerm="none", return_flows=False, flow="llin", **param):
    """In-between frames of Iin = cat(3, frame0, frame1): FlowEminND_llin_2D_v10's level loop forward and with the frames swapped,
    then the chain of flow_interpolate for every t, all on the device with one download at the end.  param: the flow driver's
    parameters; the chain's go in interp=dict(...), fill_with="nearest" and its max_dist among them.  Returns the list of frames [rows, cols(, channels)], one per t (values on Iin's
    scale); with return_flows also the forward and the backward flow as [rows, cols, 2] arrays.
    flow="tvl1": both flows by FlowTVL1's level loop instead (param: its parameters; a colour pair's flows from its gray pair)."""
    who = "interpolate_frames"
    if flow not in ("llin", "tvl1"):
        raise ValueError("%s: flow must be 'llin' or 'tvl1' (got %r)" % (who, flow))
    if flow == "tvl1":
        return _interpolate_frames_tvl1(who, Iin, channels, t, mode, return_flows, dict(param))
    param = dict(param)
    interp = dict(param.pop("interp", None) or {})
    interp.pop("mode", None)
    _, prm_kw = _interp_param(who, interp)
    times = [_time(who, x) for x in (t if np.ndim(t) else (t,))]
    scales = param.pop("scales", None)
    p = dict(ND_DEFAULTS, **param)
    p["sndTerm"] = sndTerm.lower()
    I0, I1 = _frames(Iin, channels)
    f0, f1 = dev.div_scalar(I0, 255.0), dev.div_scalar(I1, 255.0)
    Uf, Vf = _flow_llin_planes(fl.FlowLlinLevel, f0, f1, fstTerm, sndTerm, p, mode, scales=scales)
    Ub, Vb = _flow_llin_planes(fl.FlowLlinLevel, f1, f0, fstTerm, sndTerm, p, mode, scales=scales)
    Uf, Vf, Ub, Vb = (x.contiguous() for x in (Uf, Vf, Ub, Vb))
    frames = [dev.flow_interpolate(I0, I1, Uf, Vf, Ub, Vb, t=x, flow=False, source=False, mode=mode, **prm_kw)[0] for x in times]
    dev.sync_check()
    out = [dev.to_matlab(f) for f in frames]
    if channels == 1:
        out = [f[:, :, 0] for f in out]
    if return_flows:
        both = lambda a, b: np.stack([dev.to_matlab(a), dev.to_matlab(b)], axis=2)
        return out, both(Uf, Vf), both(Ub, Vb)
    return out


def _interpolate_frames_tvl1(who, Iin, channels, t, mode, return_flows, param):
    interp = dict(param.pop("interp", None) or {})
    interp.pop("mode", None)
    _, prm_kw = _interp_param(who, interp)
    times = [_time(who, x) for x in (t if np.ndim(t) else (t,))]
    p = _tvl1_param(who, param)
    I0, I1 = _frames(Iin, channels)
    g0, g1 = _tvl1_frames(_tvl1_gray_pair(who, Iin, channels))
    Uf, Vf = _flow_tvl1_planes(g0, g1, p)
    Ub, Vb = _flow_tvl1_planes(g1, g0, p)
    Uf, Vf, Ub, Vb = (x.contiguous() for x in (Uf, Vf, Ub, Vb))
    frames = [dev.flow_interpolate(I0, I1, Uf, Vf, Ub, Vb, t=x, flow=False, source=False, mode=mode, **prm_kw)[0] for x in times]
    dev.sync_check()
    out = [dev.to_matlab(f) for f in frames]
    if channels == 1:
        out = [f[:, :, 0] for f in out]
    if return_flows:
        both = lambda a, b: np.stack([dev.to_matlab(a), dev.to_matlab(b)], axis=2)
        return out, both(Uf, Vf), both(Ub, Vb)
    return out


# ---- exact Euclidean distance transform: bwdist, signed distance, nearest fill (include/pdeip.h; this library's own calls) ----
def _edt_planes(who, A):
    a = np.asfortranarray(np.asarray(A, dtype=np.float32))
    if a.ndim not in (2, 3):
        raise ValueError("%s: the input must be [rows, cols] or [rows, cols, frames] (got %s)" % (who, a.shape))
    return a, a.shape[0], a.shape[1], (a.shape[2] if a.ndim == 3 else 1)


def bwdist(BW):
    """[D, IDX] = bwdist(BW) with the Euclidean metric, one pdeip_bwdist call.  BW [rows, cols(, frames)]: a logical array, or numbers
    of which the positive ones are the features (as bwlabel takes them).  Returns (D single: the distance to the nearest feature, IDX
    int32: its 0-based column-major linear index within the frame; MATLAB's is 1-based).  Among equidistant features the lowest index
    wins.  A frame without a feature is +Inf and -1."""
    B = np.asarray(BW)
    a, rows, cols, F = _edt_planes("bwdist", (B > 0).astype(np.float32))
    D = np.empty(a.shape, np.float32, order="F")
    IDX = np.empty(a.shape, np.int32, order="F")
    capi.call("pdeip_bwdist", a.ctypes.data, rows, cols, F, D.ctypes.data, IDX.ctypes.data)
    return D, IDX


def signed_distance(A, max_dist=0):
    """The signed Euclidean distance of the level set whose inside is A >= 0, one pdeip_signed_distance call: positive inside, negative
    outside, the interface half-way between an inside pixel and its outside neighbour (so |out| >= 0.5).  The usual start of a level
    set: GAC_v10a(I, signed_distance(PHI)) where runme.m hands over PHI = +-1 and lets Reinit straighten a band of ten pixels.
    max_dist = R > 0 looks R pixels far and saturates at +-(R + 0.5) beyond; otherwise a plane without an interface is +-Inf.
    A [rows, cols(, frames)]; returns single."""
    a, rows, cols, F = _edt_planes("signed_distance", A)
    out = np.empty(a.shape, np.float32, order="F")
    capi.call("pdeip_signed_distance", a.ctypes.data, rows, cols, F, int(max_dist), out.ctypes.data)
    return out


def nearest_fill(D, max_dist=0, return_filled=False, return_dist=False):
    """Fill the holes (NaN) of the sparse map D [rows, cols(, frames)] with the nearest known pixel of the same frame, one
    pdeip_nearest_fill call: known pixels keep their bits, ties go to the lowest column-major index, a hole without a source (an empty
    frame, or none within max_dist > 0 pixels) stays NaN.  The cheapest well-defined fill -- thin cracks, the holes of a splat -- and
    NOT a substitute for TVinpaint4 on occlusion bands, whose nearest neighbour is the foreground.  Returns the filled map, with
    return_filled also the plane that is 1 on the filled holes, with return_dist also the distance to the source."""
    d, rows, cols, F = _edt_planes("nearest_fill", D)
    out = np.empty(d.shape, np.float32, order="F")
    filled = np.empty(d.shape, np.float32, order="F") if return_filled else None
    dist = np.empty(d.shape, np.float32, order="F") if return_dist else None
    capi.call("pdeip_nearest_fill", d.ctypes.data, rows, cols, F, int(max_dist), out.ctypes.data, _ptr(filled), _ptr(dist))
    res = (out,) + ((filled,) if return_filled else ()) + ((dist,) if return_dist else ())
    return res[0] if len(res) == 1 else res


# ---- primal-dual total variation: TV-L1, ROF, Huber-TV (include/pdeip.h; this library's own call) ----
def _tvpd_inputs(who, I, u0):
    f, rows, cols, F = _edt_planes(who, I)
    s = None
    if u0 is not None:
        s = np.asfortranarray(np.asarray(u0, dtype=np.float32))
        if s.shape != f.shape:
            raise ValueError("%s: u0 is %s but the input is %s" % (who, s.shape, f.shape))
    return f, s, rows, cols, F


def TVdenoisePD(I, model="l1", lam=0.8, iter=300, huber=0.0, u0=None, tau=None, sigma=None):
    """Total-variation denoising by the first-order primal-dual iteration of Chambolle and Pock, resident on the device
    (device.tv_pd).  I [rows, cols(, frames)] of any numeric type, taken as single; NaN means no data.  model 'l1': TV + lam |u - I|,
    which rejects gross outliers where a quadratic data term averages them in; 'l2': TV + lam/2 (u - I)^2 (ROF); huber > 0: the Huber
    norm in place of TV, which takes the staircase out of slopes.  The start is u0, or I with its holes filled from the nearest known
    pixel.  tau, sigma: None = 0.25 and 0.5 (tau sigma 8 <= 1).  No pyramid, no linear solver, no eps.  Returns single."""
    who = "TVdenoisePD"
    prm = dev.TvpdParams.make(model, lam, iter, huber, tau, sigma, who=who)
    f, s, _, _, _ = _tvpd_inputs(who, I, u0)
    out = dev.tv_pd(dev.to_device(f), prm.model, lam, iter, huber, None if s is None else dev.to_device(s), tau, sigma)
    dev.sync_check()
    return dev.to_matlab(out)


def capi_TVdenoisePD(I, model="l1", lam=0.8, iter=300, huber=0.0, u0=None, tau=None, sigma=None):
    """pdeip_tv_pd on MATLAB-shaped numpy arrays: TVdenoisePD through the host entry point, same bits."""
    who = "capi_TVdenoisePD"
    prm = dev.TvpdParams.make(model, lam, iter, huber, tau, sigma, who=who)
    f, s, rows, cols, F = _tvpd_inputs(who, I, u0)
    out = np.empty(f.shape, np.float32, order="F")
    capi.call("pdeip_tv_pd", f.ctypes.data, _ptr(s), rows, cols, F, ctypes.addressof(prm), out.ctypes.data)
    return out


# ---- TV-L1 optical flow: primal-dual, warped, coarse to fine (include/pdeip.h; this library's own driver) ----
TVL1_DEFAULTS = dict(lam=15.0, warps=3, iter=20, huber=0.0, scl_factor=0.75, scales=None, tau=None, sigma=None)


def _tvl1_param(who, param):
    unknown = sorted(set(param) - set(TVL1_DEFAULTS))
    if unknown:
        raise ValueError("%s: unknown parameter %s (of %s)" % (who, ", ".join(unknown), ", ".join(sorted(TVL1_DEFAULTS))))
    p = dict(TVL1_DEFAULTS, **param)
    if not int(p["warps"]) > 0 or not int(p["iter"]) > 0 or not float(p["lam"]) > 0:
        raise ValueError("%s: lam, warps and iter must be positive" % who)
    return p


def _tvl1_gray_pair(who, Iin, channels):
    """Both frames of Iin = cat(3, frame0, frame1), 0..255, as resident gray planes [1, ncols, nrows] ./ 255; a colour pair's gray value
    is ((R + G) + B) / 3 in float32, formed on the host."""
    I = np.asarray(Iin, dtype=np.float32)
    if channels not in (1, 3) or I.ndim != 3 or I.shape[2] != 2 * channels:
        raise ValueError("%s: Iin must be [rows, cols, 2 * channels] with channels 1 or 3 (got %s, channels %r)" % (who, I.shape, channels))
    if I.shape[0] < 2 or I.shape[1] < 2:
        raise ValueError("%s: the frames must be at least 2x2 (got %s)" % (who, I.shape[:2]))
    if channels == 3:
        three = np.float32(3.0)
        I = np.stack([((I[:, :, 0] + I[:, :, 1]) + I[:, :, 2]) / three, ((I[:, :, 3] + I[:, :, 4]) + I[:, :, 5]) / three], axis=2)
    return I


def _tvl1_frames(gray):
    I0, I1 = _frames(gray, 1)
    return dev.div_scalar(I0, 255.0), dev.div_scalar(I1, 255.0)


def _flow_tvl1_planes(f0, f1, p):
    """The level loop of FlowTVL1 on resident gray frames f0, f1 [1, ncols, nrows] (already ./255): the flow as two resident planes."""
    P0, P1 = pyramid.build_dev(f0, f1, p["scl_factor"], 20, max_scales=p["scales"])
    level = fl.FlowTvl1Level(p)
    U = _zeros_like_plane(P0[-1])
    V = torch.zeros_like(U)
    for scl in range(len(P0) - 1, -1, -1):
        U, V = level.run(P0[scl], P1[scl], U, V)
        if scl > 0:
            cols, rows = P0[scl - 1].shape[-2:]
            U, V = _up(U, 1.0 / p["scl_factor"], rows, cols), _up(V, 1.0 / p["scl_factor"], rows, cols)
    return U, V


def FlowTVL1(Iin, channels=1, **param):
    """[U V] = TV-L1 optical flow of Iin = cat(3, frame0, frame1), values 0..255: Zach, Pock and Bischof's model by Chambolle and Pock's
    primal-dual iteration, warped and coarse to fine on the late-linearisation drivers' pyramid, resident on the device
    (pyramid.build_dev and flow_level.FlowTvl1Level).  param: lam (15), warps (3) per scale, iter (20) per warp, huber (0 = TV),
    scl_factor (0.75), scales (all), tau, sigma (0.25, 0.5).  channels = 3: the flow of the gray pair ((R + G) + B) / 3.  No linear
    solver and no ordering: `mode` does not apply.  Returns U (along the columns) and V (down the rows), single [rows, cols]."""
    who = "FlowTVL1"
    p = _tvl1_param(who, dict(param))
    U, V = _flow_tvl1_planes(*_tvl1_frames(_tvl1_gray_pair(who, Iin, channels)), p)
    dev.sync_check()
    return dev.to_matlab(U), dev.to_matlab(V)


def capi_FlowTVL1(Iin, channels=1, **param):
    """pdeip_flow_tvl1 on MATLAB-shaped numpy arrays: FlowTVL1 through the host entry point, one resident run, same bits.  The C-ABI
    takes the gray pair; a colour pair's is formed here as in FlowTVL1."""
    who = "capi_FlowTVL1"
    p = _tvl1_param(who, dict(param))
    g = np.asfortranarray(_tvl1_gray_pair(who, Iin, channels), dtype=np.float32)
    rows, cols = g.shape[:2]
    nan = float("nan")
    d = lambda v: nan if v is None else float(v)
    prm = dev.FlowTvl1Params(float(p["lam"]), float(p["huber"]), d(p["tau"]), d(p["sigma"]), float(p["scl_factor"]), int(p["warps"]), int(p["iter"]),
                             0 if p["scales"] is None else int(p["scales"]))
    U, V = np.empty((rows, cols), np.float32, order="F"), np.empty((rows, cols), np.float32, order="F")
    capi.call("pdeip_flow_tvl1", g.ctypes.data, rows, cols, ctypes.addressof(prm), U.ctypes.data, V.ctypes.data)
    return U, V
