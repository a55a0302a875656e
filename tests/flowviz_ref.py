"""NumPy float64 restatement of flow2color (matlab/optical_flow/flow2color.m) and of the flow error measures, as include/pdeip.h
defines them: the inputs are float32 promoted to float64, every step is a float64 operation in the order written here, the picture is
rounded once to float32, and the uint8 picture is uint8(round(255 x)) of that float32 value.

tests/test_flowviz_ref.py checks this file against known answers; tests/test_gpu_flowviz.py compares the GPU with it."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
TWO_PI = 2.0 * math.pi
DEG_PER_RAD = 180.0 / math.pi


def hsv2rgb(h, s, v):
    """The six-sector formula on arrays: k = floor(6 h) (6 taken as 0), f = 6 h - k, p = v (1 - s), q = v (1 - s f),
    t = v (1 - s (1 - f)); sector k picks (v,t,p) (q,v,p) (p,v,t) (p,q,v) (t,p,v) (v,p,q)."""
    h6 = 6.0 * h
    k = np.floor(h6)
    f = h6 - k
    k = np.where(k >= 6.0, 0.0, k).astype(np.int64)
    p, q, t = v * (1.0 - s), v * (1.0 - s * f), v * (1.0 - s * (1.0 - f))
    r = np.choose(k, [v, q, p, p, t, v])
    g = np.choose(k, [t, v, v, q, p, p])
    b = np.choose(k, [p, p, t, v, v, q])
    return r, g, b


def max_magnitude(U, V):
    """MATLAB's max(mag(:)): NaNs ignored, Inf counts, all-NaN gives NaN."""
    U, V = np.asarray(U, F32).astype(F64), np.asarray(V, F32).astype(F64)
    with np.errstate(all="ignore"):
        mag = np.sqrt(U * U + V * V)
    ok = ~np.isnan(mag)
    return float(mag[ok].max()) if ok.any() else math.nan


def _code(U, V, maxvalue):
    """flow2color.m:38-59 on float64 arrays: the float64 (r, g, b) and the valid mask."""
    with np.errstate(all="ignore"):
        d = np.arctan2(-V, -U)
        d = np.where(d < 0.0, d + TWO_PI, d)
        d = d / TWO_PI
        mag = np.sqrt(U * U + V * V) / maxvalue
        mag = np.where(mag > 1.0, 1.0, mag)
        valid = np.isfinite(U) & (mag <= 1.0)
    h = np.where(valid, d, 1.0)
    s = np.where(valid, 1.0, 0.0)
    v = np.where(valid, mag, 1.0)
    return hsv2rgb(h, s, v), valid


def frame_field(brows, bcols):
    """The synthetic field of flow2color.m:30-33 (1-based meshgrid)."""
    j, i = np.meshgrid(np.arange(1, bcols + 1, dtype=F64), np.arange(1, brows + 1, dtype=F64))
    return (j / bcols - 0.5) * 10.0, (i / brows - 0.5) * 10.0


def flow2color(U, V, maxvalue=None, border=0, detail=False):
    """img float32 [rows + 2 border, cols + 2 border, 3] and the maximum used.  detail=True: also the float64 picture and the
    valid mask of the flow's own pixels."""
    U, V = np.asarray(U, F32).astype(F64), np.asarray(V, F32).astype(F64)
    rows, cols = U.shape
    if maxvalue is None or (isinstance(maxvalue, float) and math.isnan(maxvalue)):
        maxvalue = max_magnitude(U, V)
    maxvalue = float(maxvalue)
    (r, g, b), valid = _code(U, V, maxvalue)
    inner = np.stack([r, g, b], axis=2)
    if border > 0:
        brows, bcols = rows + 2 * border, cols + 2 * border
        X, Y = frame_field(brows, bcols)
        fmax = float(np.sqrt(X * X + Y * Y).max())  # by brute force; the library uses the closed form sqrt(50)
        (fr, fg, fb), _ = _code(X, Y, fmax)
        img = np.stack([fr, fg, fb], axis=2)
        o = border - 1  # imgOut(border:border+rows-1, ...) is 1-based
        img[o:o + rows, o:o + cols, :] = inner
    else:
        img = inner
    out = np.asfortranarray(img.astype(F32))
    if detail:
        return out, maxvalue, img, valid
    return out, maxvalue


def to_uint8(img32):
    """uint8(round(255 x)) of the float32 picture: 255 x and + 0.5 are exact in float64, so floor(y + 0.5) is MATLAB's round for
    x >= 0; saturating.  Same [rows, cols, 3] indexing; C order is the interleaved row-major picture."""
    y = np.floor(255.0 * np.asarray(img32, F32).astype(F64) + 0.5)
    return np.ascontiguousarray(np.clip(y, 0.0, 255.0).astype(np.uint8))


def flow_errors(U, V, Ut, Vt, mask=None):
    """dict: epe, ang float32 planes (NaN where a pixel does not count), counted (bool), epe64 / ang64 the float64 values of the
    counted pixels in column-major order, count, mean_epe, mean_ang (math.fsum / count), max_epe; NaN statistics with count 0."""
    U, V, Ut, Vt = [np.asarray(a, F32).astype(F64) for a in (U, V, Ut, Vt)]
    counted = np.isfinite(U) & np.isfinite(V) & np.isfinite(Ut) & np.isfinite(Vt)
    if mask is not None:
        counted &= np.asarray(mask, F32) != 0
    with np.errstate(all="ignore"):
        du, dv = U - Ut, V - Vt
        epe = np.sqrt(du * du + dv * dv)
        c = (U * Ut + V * Vt + 1.0) / (np.sqrt(U * U + V * V + 1.0) * np.sqrt(Ut * Ut + Vt * Vt + 1.0))
        c = np.where(c < -1.0, -1.0, np.where(c > 1.0, 1.0, c))
        ang = np.arccos(c) * DEG_PER_RAD
    epe = np.where(counted, epe, np.nan)
    ang = np.where(counted, ang, np.nan)
    e64, a64 = epe.T[counted.T], ang.T[counted.T]
    n = int(counted.sum())
    return dict(epe=np.asfortranarray(epe.astype(F32)), ang=np.asfortranarray(ang.astype(F32)), counted=counted, epe64=e64, ang64=a64,
                epe_plane64=epe, ang_plane64=ang, count=n, mean_epe=math.fsum(e64) / n if n else math.nan, mean_ang=math.fsum(a64) / n if n else math.nan,
                max_epe=float(e64.max()) if n else math.nan)
