"""Solver inputs laced with the values at the edges of float32's range: divisor data of +-3e38 and +Inf (the denominator is
>= 2^126, its reciprocal subnormal or zero), weights that are exactly 0.0f and -0.0f, subnormal and negative-zero right-hand
sides and iterates, NaN -- and, on request, one pixel whose denominator is subnormal, so that its reciprocal overflows.

tests/problems.py draws ordinary numbers (weights in [0.5, 5], data terms in [0.05, 2.3], TRACE = 1 + sum(w)) and NaN, so
every divisor a kernel derives from it lies between about 2 and 25.  range_laced() takes such a problem without NaN and
overwrites planes pixel by pixel.  ONE uniform plane decides the class of a pixel, so the classes are disjoint, NaN included:
a NaN divisor plane on top of an overwritten right-hand side (or zero weights under a NaN TRACE, where 1/0 floods forward)
leaves few finite outputs in lexicographic order, and a comparison in which any NaN equals any NaN then proves little.
A class holds for all frames of a pixel, and for both fields of the symmetric disparity problem.

    class    planes                                                    value
    H+ H- I  the divisor data planes (Du, Dv / Du / TRACE)             3e38f, -3e38f, +Inf
    Z  Z-    all four (eight) weights                                  0.0f, -0.0f
    E0       wE only                                                   0.0f
    W-       wW only                                                   -0.0f
    C  C-    the right-hand sides (Cu, Cv, M / Cu / B)                 1e-41f, -0.0f
    X  X-    the iterate planes                                        3e-42f, -0.0f
    N        the planes problems.py laces in its "all" mode            NaN
    T        corner=True: the last relaxed pixel [-2, -2] alone        all weights 0, divisor data 1e-39f

Class T is for point SOR only, on frames of at least 8192 pixels.  Point SOR relaxes rows 1..nrows-2 and columns 1..ncols-2 and
copies the border from them, so the class sits on the last INTERIOR pixel in lexicographic order (on the border pixel [-1, -1]
it would reach no output).  There the Inf it makes stays within a triangle of `iter` pixels, while a Thomas solve carries it
along whole lines -- one such pixel makes every output of every line-relaxation gateway non-finite, in both orders.

divisors() restates, in numpy float32 and in the association order of each model's derive() (csrc/pdeip_models.hpp,
pdeip_sor_pde8.hpp), the sum whose reciprocal the point solvers take; in_fast_range() is the range in which the pipeline's
v_rcp_f32 + one Newton step equals the IEEE quotient, outside of which a wave of k_sor_rbp redoes its lanes with the division.
"""
import numpy as np

import problems as pb

F32 = np.float32
W4 = ("wW", "wN", "wE", "wS")
W8 = ("wW", "wNW", "wN", "wNE", "wE", "wSE", "wS", "wSW")
OFLOW = dict(div=("Du", "Dv"), rhs=("Cu", "Cv", "M"), nan=("M", "Cu", "Cv", "Du", "Dv"))
# model -> the planes of each role
ROLES = {
    "elin4": dict(OFLOW, w=W4, x=("U", "V")),
    "llin4": dict(OFLOW, w=W4, x=("dU", "dV")),
    "llin8": dict(OFLOW, w=W8, x=("dU", "dV")),
    "disp4": dict(div=("Du",), rhs=("Cu",), nan=("Cu", "Du"), w=W4, x=("dU",)),
    "pde4": dict(div=("TRACE",), rhs=("B",), nan=("TRACE",), w=W4, x=("X",)),
    "pde8": dict(div=("TRACE",), rhs=("B",), nan=("TRACE",), w=W8, x=("X",)),
}
ROLES["dispsym4"] = {role: tuple(k + s for s in "01" for k in names) for role, names in ROLES["disp4"].items()}
MODELS = tuple(ROLES)
DIV_CLASSES = ("H+", "H-", "I")
CLASSES = DIV_CLASSES + ("Z", "Z-", "E0", "W-", "C", "C-", "X", "X-")  # then N, at nan_frac
# class -> (role or plane names, value)
VALUES = {"H+": ("div", F32(3e38)), "H-": ("div", F32(-3e38)), "I": ("div", F32(np.inf)), "Z": ("w", F32(0.0)), "Z-": ("w", F32(-0.0)),
          "E0": ("wE", F32(0.0)), "W-": ("wW", F32(-0.0)), "C": ("rhs", F32(1e-41)), "C-": ("rhs", F32(-0.0)), "X": ("x", F32(3e-42)),
          "X-": ("x", F32(-0.0)), "N": ("nan", F32(np.nan))}
CORNER_MIN_PIXELS = 8192
CORNER = (-2, -2)  # the last pixel point SOR relaxes


def _planes(model, what):
    roles = ROLES[model]
    if what in roles:
        return roles[what]
    return tuple(what + s for s in "01") if model == "dispsym4" else (what,)  # a single weight plane


def class_map(seed, nrows, ncols, frac=0.01, div_frac=None, nan_frac=0.02):
    """-> {class: boolean [nrows, ncols] mask}, disjoint: consecutive intervals of one uniform plane."""
    div_frac = frac if div_frac is None else div_frac
    shares = [(c, div_frac if c in DIV_CLASSES else frac) for c in CLASSES] + [("N", nan_frac)]
    assert sum(s for _, s in shares) <= 1.0, "the classes' shares exceed the frame"
    u = np.random.default_rng([seed, 0x72616e67]).uniform(size=(nrows, ncols))
    masks, lo = {}, 0.0
    for c, s in shares:
        masks[c] = (u >= lo) & (u < lo + s)
        lo += s
    return masks


def range_laced(model, seed, nrows, ncols, nframes=1, frac=0.01, div_frac=None, nan_frac=0.02, corner=False):
    """The model's problems.py problem (no NaN of its own) with the classes of the table written over it."""
    if model in ("disp4", "dispsym4"):
        assert nframes == 1
        p = getattr(pb, model)(seed, nrows, ncols)
    else:
        p = getattr(pb, model)(seed, nrows, ncols, nframes)
    masks = class_map(seed, nrows, ncols, frac, div_frac, nan_frac)
    if corner:
        assert nrows * ncols >= CORNER_MIN_PIXELS, "class T needs a frame of at least %d pixels" % CORNER_MIN_PIXELS
        for m in masks.values():
            m[CORNER] = False
    for c, m in masks.items():
        what, value = VALUES[c]
        for k in _planes(model, what):
            p[k][m] = value  # [nrows, ncols] mask on [nrows, ncols(, nframes)]: every frame of the pixel
    if corner:
        for k in _planes(model, "w"):
            p[k][CORNER] = F32(0.0)
        for k in _planes(model, "div"):
            p[k][CORNER] = F32(1e-39)
    return p


def _holds(a, value):
    """[nrows, ncols] mask: the plane holds `value` -- same bits, or NaN for NaN -- in every frame of the pixel."""
    m = np.isnan(a) if np.isnan(value) else (a.view(np.uint32) == np.asarray(value, F32).view(np.uint32))
    return m.all(axis=2) if m.ndim == 3 else m


def census(model, p):
    """-> {class: pixels that hold it}, read off the PLANES of the problem: a pixel counts for a class when every plane of the
    class's role holds the class's value there, in every frame.  Z / Z- also hold E0's / W-'s value on that one plane, so E0 and W-
    count only the pixels whose other weights are not zero; T is the pixel with zero weights and divisor data of 1e-39f."""
    out = {}
    all_w = [p[k] for k in _planes(model, "w")]
    zero_w = np.logical_and.reduce([_holds(a, F32(0.0)) | _holds(a, F32(-0.0)) for a in all_w])
    for c, (what, value) in VALUES.items():
        m = np.logical_and.reduce([_holds(p[k], value) for k in _planes(model, what)])
        if c in ("E0", "W-"):
            m = m & ~zero_w
        out[c] = int(m.sum())
    t = zero_w & np.logical_and.reduce([_holds(p[k], F32(1e-39)) for k in _planes(model, "div")])
    if t.any():
        out["T"] = int(t.sum())
        out["Z"] -= int((t & np.logical_and.reduce([_holds(a, F32(0.0)) for a in all_w])).sum())
    return out


def _frame0(a):
    return a[..., 0] if a.ndim == 3 else a


def divisors(model, p):
    """The sum each derive() feeds its reciprocal, float32, one plane per divisor stacked along a new first axis: (Du-, Dv-divisor)
    for the coupled models, which read frame 0 of their data terms; one for disp4 and for every frame of pde4 / pde8; the two
    fields' for dispsym4."""
    with np.errstate(all="ignore"):
        if model in ("elin4", "llin4", "llin8"):  # ModelElin4::derive: (wW + wE) + (wN + wS), then + Du unless Du is NaN
            t1 = (p["wW"] + p["wE"]) + (p["wN"] + p["wS"])
            return np.stack([np.where(np.isnan(d), t1, t1 + d) for d in (_frame0(p["Du"]), _frame0(p["Dv"]))])
        if model == "disp4":  # ModelDisp4::derive: (((Du + wE) + wW) + wS) + wN, Du left out where Cu is NaN
            t = np.where(np.isnan(p["Cu"]), p["wE"], p["Du"] + p["wE"])
            return (((t + p["wW"]) + p["wS"]) + p["wN"])[None]
        if model == "dispsym4":
            return np.concatenate([divisors("disp4", {k[:-1]: v for k, v in p.items() if k.endswith(s)}) for s in "01"])
        tr = p["TRACE"]
        w = lambda k: p[k][..., None] if tr.ndim == 3 and p[k].ndim == 2 else p[k]
        t = (w("wE") + w("wW")) + (w("wS") + w("wN"))
        if model == "pde8":  # p8_derive
            t = (t + (w("wSW") + w("wNW"))) + (w("wSE") + w("wNE"))
        return np.where(np.isnan(tr), t, tr).astype(F32)[None]


def in_fast_range(d):
    """2^-126 <= |d| < 2^126: RcpRange of csrc/pdeip_models.hpp (NaN, zero, infinities and subnormals are outside)."""
    a = np.abs(np.asarray(d, dtype=F32))
    return (a >= F32(2.0 ** -126)) & (a < F32(2.0 ** 126))


def fallback_group_share(model, p, own_rows=240):
    """Share of the (column, `own_rows`-row tile[, frame]) groups that hold a divisor outside the fast range: about the share of
    k_sor_rbp's waves that take the IEEE division in the first sweep (the 16 halo lanes of a wave are left out)."""
    bad = ~in_fast_range(divisors(model, p))
    bad = bad.any(axis=0)  # a pixel with either divisor outside
    bad = bad.reshape(bad.shape[0], -1)  # frames side by side as further columns
    tiles = [bad[r:r + own_rows].any(axis=0) for r in range(0, bad.shape[0], own_rows)]
    return float(np.mean(np.concatenate(tiles)))
