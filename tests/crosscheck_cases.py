"""The seeded cases of the cross-check tests, shared by the CPU half (test_crosscheck_ref.py) and the GPU half
(test_gpu_crosscheck.py).  A case is a set of column-major float32 planes and the parameter sets it runs with.

Shapes: the smallest at which the indexing can go wrong -- the narrowest plane the calls accept, a single row, a column longer than a
workgroup (257 rows: lanes 0 and 256 of two workgroups), a plane that is no multiple of anything, and one of many workgroups.
The laced pixels sit at the first pixel, the last pixel and on both sides of the 64- and 256-lane seams, counted along the plane's
memory order (rows 63 | 64 and 255 | 256 of the first column where the column is that long) and again in the second column."""
import numpy as np

F32 = np.float32

DISP_SHAPES = [(1, 2), (7, 2), (1, 300), (257, 3), (37, 53), (270, 480)]
FLOW_SHAPES = [(2, 2), (7, 2), (2, 300), (257, 3), (37, 53), (270, 480)]
DISP_KINDS = ["normal", "nonfinite_checked", "nonfinite_gathered", "neg_zero", "edges", "zero_weight_nan", "all_nan", "constant"]
FLOW_KINDS = ["normal", "nonfinite_checked", "nonfinite_gathered", "neg_zero", "edges", "zero_weight_nan", "all_nan", "constant"]


def shape_id(s):
    return "%dx%d" % s


def lace_positions(shape):
    rows, cols = shape
    n = rows * cols
    at = {0, n - 1, 63, 64, 255, 256}
    if cols > 1:
        at |= {rows + k for k in (0, 63, 64, 255, 256) if k < rows}
    return sorted(k for k in at if 0 <= k < n)


def disp_is_big(shape):
    """The 'normal' disparity cases that must exercise both branches: at least 300 pixels and 50 columns."""
    return shape[0] * shape[1] >= 300 and shape[1] >= 50


def flow_is_big(shape):
    """The same for the flow, whose query also moves along y: at least 30 rows as well."""
    return disp_is_big(shape) and shape[0] >= 30


def normal_fields(shape):
    """D0, D1, Uf, Vf, Ub, Vb drawn in this order from one generator; amplitude 2, or 0.3 on the tiny shapes so that some queries stay
    in range."""
    rng = np.random.default_rng(11 + 1000 * shape[0] + shape[1])
    raw = [rng.normal(size=shape) for _ in range(6)]
    da = 2.0 if disp_is_big(shape) else 0.3
    fa = 2.0 if flow_is_big(shape) else 0.3
    amp = [da, da, fa, fa, fa, fa]
    return [np.asfortranarray((a * r).astype(F32)) for a, r in zip(amp, raw)]


def _flat(A):
    return A.reshape(-1, order="F")   # a view of a column-major plane


def _lace(A, values, at):
    f = _flat(A)
    for k, p in enumerate(at):
        f[p] = values[k % len(values)]


def _on_the_edges(shape, axis, step=1):
    """Displacements that put the query exactly on the last line (s = 1), exactly on the first, and one float32 ulp outside each,
    by (i + step j) % 4.  axis 1: along x (the query is (j+1) + d); axis 0: along y."""
    rows, cols = shape
    i, j = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    pos = (j if axis == 1 else i).astype(F32)
    last = F32(cols if axis == 1 else rows)
    to_last, to_first = last - (pos + F32(1)), -pos
    kind = (i + step * j) % 4
    d = np.where(kind == 0, to_last, np.where(kind == 1, to_first, np.where(kind == 2, np.nextafter(to_last, F32(np.inf)),
                                                                            np.nextafter(to_first, F32(-np.inf)))))
    return np.asfortranarray(d.astype(F32))


def disp_case(shape, kind):
    """-> (D0, D1, tols)."""
    D0, D1 = normal_fields(shape)[:2]
    at = lace_positions(shape)
    tols = [2.0]
    if kind == "normal":
        tols = [2.0, 0.0, np.inf]
    elif kind == "nonfinite_checked":
        _lace(D0, [np.nan, np.inf, -np.inf], at)
    elif kind == "nonfinite_gathered":   # their neighbours' queries pick them up
        _lace(D1, [np.nan, -np.inf, np.inf], at)
    elif kind == "neg_zero":             # -0.0 against +-0.0: r = +-0, kept even at tol = 0, and the sparse map keeps the sign bit
        _lace(D0, [-0.0], at)
        _lace(D1, [-0.0, 0.0], at)
        tols = [2.0, 0.0]
    elif kind == "edges":
        D0 = _on_the_edges(shape, 1)
        tols = [np.inf, 2.0]
    elif kind == "zero_weight_nan":      # integer disparities: s = 0, and the right tap's weight is 0 whatever it holds
        rng = np.random.default_rng(5 + shape[0])
        D0 = np.asfortranarray(rng.integers(-2, 3, size=shape).astype(F32))
        _lace(D1, [np.nan], at)
        D1[:, shape[1] // 2] = np.nan
        tols = [np.inf, 2.0]
    elif kind == "all_nan":
        D0[...] = np.nan
        D1[...] = np.nan
    elif kind == "constant":             # d against -d: r == 0 exactly wherever the query is in range
        D0[...] = 1.0
        D1[...] = -1.0
        tols = [0.0]
    else:
        raise ValueError(kind)
    return D0, D1, tols


def flow_case(shape, kind):
    """-> (Uf, Vf, Ub, Vb, [(a, b), ..])."""
    Uf, Vf, Ub, Vb = normal_fields(shape)[2:]
    at = lace_positions(shape)
    ab = [(0.5, 2.0)]
    if kind == "normal":
        ab = [(0.5, 2.0), (0.01, 0.5), (0.0, 1.0), (0.0, 0.0), (0.0, np.inf)]
    elif kind == "nonfinite_checked":
        _lace(Uf, [np.nan, np.inf, -np.inf], at)
        _lace(Vf, [-np.inf, np.nan, 1.0], at[::2])
    elif kind == "nonfinite_gathered":
        _lace(Ub, [np.nan, -np.inf, np.inf], at)
        _lace(Vb, [np.inf, np.nan], at[1::2])
    elif kind == "neg_zero":
        for P, vals in ((Uf, [-0.0]), (Vf, [-0.0, 0.0]), (Ub, [0.0, -0.0]), (Vb, [-0.0])):
            _lace(P, vals, at)
        ab = [(0.5, 2.0), (0.0, 0.0)]
    elif kind == "edges":
        Uf, Vf = _on_the_edges(shape, 1), _on_the_edges(shape, 0, step=2)   # every pairing of the four kinds occurs
        ab = [(0.0, np.inf), (0.5, 2.0)]
    elif kind == "zero_weight_nan":
        rng = np.random.default_rng(5 + shape[0])
        Uf = np.asfortranarray(rng.integers(-1, 2, size=shape).astype(F32))
        Vf = np.asfortranarray(rng.integers(-1, 2, size=shape).astype(F32))
        _lace(Ub, [np.nan], at)
        Ub[:, shape[1] // 2] = np.nan
        Vb[shape[0] // 2, :] = np.nan
        ab = [(0.0, np.inf), (0.5, 2.0)]
    elif kind == "all_nan":
        for P in (Uf, Vf, Ub, Vb):
            P[...] = np.nan
    elif kind == "constant":             # (1, -1) against (-1, 1): e == 0 exactly wherever the query is in range
        Uf[...] = 1.0
        Vf[...] = -1.0
        Ub[...] = -1.0
        Vb[...] = 1.0
        ab = [(0.0, 0.0)]
    else:
        raise ValueError(kind)
    return Uf, Vf, Ub, Vb, ab
