"""Helpers shared by the GPU tests of the flow tools (test_gpu_flowviz.py, test_gpu_crosscheck.py, test_gpu_flow_rounds.py): planes
carved at a 4-byte offset, bit comparisons, the float picture's and the angular error's tolerances, the runs and checks of
pdeip_flow_errors_dev, and the statistics of both units against the documented sum order (reduce_tree_ref.py)."""
import importlib
import math

import numpy as np

import flowviz_ref as fr
import reduce_tree_ref as rt

F32, F64 = np.float32, np.float64


def _dev():
    return importlib.import_module("pde-based-image-processing_amd.device")


RGB_TOL = 2.0 ** -24
# The relative difference between the device's double acos and the host libm's, argument identical.  No ulp statement for the device
# math library ships with the toolchain, so the figure was measured once on the MI355X (23 205 pixels of these cases'
# fields, random, nearly parallel and nearly opposite pairs, each pixel's float64 value read through a one-pixel mask): 2.48e-16 =
# 2^-51.84, a little over one ulp.  The bound is four times that (another libm version has to pass too), never looser than 2^-40.
ANG_MEASURED = 2.48e-16
ANG_TOL = min(4.0 * ANG_MEASURED, 2.0 ** -40)


def carve(a, offset):
    """The plane on the device, [ncols, nrows]; offset 1: at 4 bytes past a 16-byte boundary."""
    import torch

    t = _dev().to_device(a)
    if not offset:
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=t.device)
    assert buf.data_ptr() % 16 == 0
    out = buf[1:1 + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def same_f32(got, want, what):
    assert got.shape == want.shape and got.dtype == F32, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaN at %d pixels where the restatement has none or the reverse" % (what, int((gn != wn).sum()))
    bad = got[~gn].view(np.uint32) != want[~wn].view(np.uint32)
    assert not bad.any(), "%s: %d values differ in their bits" % (what, int(bad.sum()))


def _bits(x):
    return np.float64(x).view(np.uint64)


def _same_max(got, want, what):
    assert (math.isnan(got) and math.isnan(want)) or _bits(got) == _bits(want), "%s: maxvalue %r != %r" % (what, got, want)


def check_rgb(got, ref32, exact, what):
    assert got.shape == ref32.shape and got.dtype == F32, what
    diff = np.abs(got.astype(F64) - ref32.astype(F64))
    assert not np.isnan(diff).any() and diff.max() <= RGB_TOL, "%s: float rgb off by %.3g" % (what, diff.max())
    assert np.array_equal(got[exact], ref32[exact]), "%s: invalid / zero-magnitude pixels differ" % what


def exact_mask(U, V, valid, border=0):
    """Pixels of the picture that must match to the bit: the flow's invalid and zero-magnitude ones."""
    inner = ~valid | ((U == 0) & (V == 0))
    rows, cols = U.shape
    m = np.zeros((rows + 2 * border, cols + 2 * border), bool)
    o = max(border - 1, 0)
    m[o:o + rows, o:o + cols] = inner
    return m


def ulp_mid_ok(got32, ref32, ref64, tol, what):
    """got32 equals ref32 up to the one float32 rounding: where they differ they are neighbours and the float64 value lies within
    tol (relative) of the midpoint between them."""
    off = got32 != ref32
    off &= ~(np.isnan(got32) & np.isnan(ref32))
    if off.any():
        g, r, x = got32[off].astype(F64), ref32[off].astype(F64), ref64[off]
        assert np.all(np.abs(g - r) <= np.spacing(np.maximum(np.abs(got32[off]), np.abs(ref32[off]))).astype(F64)), what + ": not neighbours"
        assert np.all(np.abs(x - 0.5 * (g + r)) <= tol * np.abs(x)), what + ": differs away from a rounding boundary"


def run_errors(pdeip, planes, mask, offset):
    import torch

    dev = _dev()
    ts = [carve(p, offset) for p in planes]
    tm = None if mask is None else carve(mask, offset)
    epe, ang, stats = dev.flow_errors(*ts, mask=tm)
    assert pdeip.capi.load().pdeip_last_launch_count() == 2
    epe2, ang2, stats2 = dev.flow_errors(*ts, mask=tm, epe_out=torch.full_like(ts[0], 5.0), ang_out=torch.full_like(ts[0], 5.0))
    torch.cuda.synchronize()
    assert pdeip.capi.last_error() == ""
    out = dev.to_matlab(epe), dev.to_matlab(ang), stats.cpu().numpy()
    assert dev.to_matlab(epe2).tobytes() == out[0].tobytes() and dev.to_matlab(ang2).tobytes() == out[1].tobytes()
    assert stats2.cpu().numpy().tobytes() == out[2].tobytes(), "two calls differ"
    return out


def check_errors(got, want, what, tree=None):
    epe, ang, stats = got
    n = want["count"]
    assert np.array_equal(np.isnan(epe), ~want["counted"]) and np.array_equal(np.isnan(ang), ~want["counted"]), what + ": excluded pixels differ"
    ok = want["counted"]
    assert np.array_equal(epe[ok].view(np.uint32), want["epe"][ok].view(np.uint32)), what + ": endpoint error bits differ"
    assert stats[0] == n, what
    if n == 0:
        assert np.isnan(stats[1:]).all(), what
        return
    assert _bits(stats[3]) == _bits(want["max_epe"]), what
    bound = 2.0 * n * 2.0 ** -53
    rel_e = abs(stats[1] - want["mean_epe"]) / want["mean_epe"] if want["mean_epe"] else abs(stats[1])
    rel_a = abs(stats[2] - want["mean_ang"]) / want["mean_ang"] if want["mean_ang"] else abs(stats[2])
    print("%s: n %d, mean endpoint error off by %.3g relative (bound %.3g), mean angular error by %.3g (bound %.3g)"
          % (what, n, rel_e, bound, rel_a, bound + ANG_TOL))
    assert rel_e <= bound
    assert rel_a <= bound + ANG_TOL
    ulp_mid_ok(ang, want["ang"], want["ang_plane64"], ANG_TOL, what + " angular error")
    # the documented order (reduce_tree_ref.py): the endpoint errors are correctly rounded on both sides, so their mean has the tree's
    # bits; the angular errors are the two libraries' acos, so the trees run over summands up to ANG_TOL apart
    tree = error_tree_of(want) if tree is None else tree
    assert stats[0] == tree["count"] and _bits(stats[3]) == _bits(tree["max_epe"]), what
    assert _bits(stats[1]) == _bits(tree["mean_epe"]), "%s: the mean endpoint error %.17g is not that of the documented order, %.17g" % (
        what, stats[1], tree["mean_epe"])
    tree_a = abs(stats[2] - tree["mean_ang"]) / tree["mean_ang"] if tree["mean_ang"] else abs(stats[2])
    assert tree_a <= ANG_TOL + 2.0 * (tree["ntiles"] + 18) * 2.0 ** -53, what + ": mean angular error against the documented order"


def error_tree_of(want):
    """The statistics in the documented order from the restatement's float64 planes, in memory order."""
    flat = lambda a: np.asarray(a).reshape(-1, order="F")
    return rt.flow_error_stats(flat(want["counted"]), flat(want["epe_plane64"]), flat(want["ang_plane64"]))


def cross_tree_of(want):
    """The statistics in the documented order (reduce_tree_ref.py) from the restatement's masks and float64 magnitudes."""
    mag = np.abs(want["r"]) if "r" in want else want["err64"]
    return rt.crosscheck_stats(want["kept_mask"], want["defined_mask"], mag, *mag.shape)


def check_stats(stats, want, what):
    tree = cross_tree_of(want)
    assert stats[0] == want["kept"] and stats[1] == want["defined"], "%s: counts %r, want %d / %d" % (what, stats[:2], want["kept"], want["defined"])
    assert tree["kept"] == want["kept"] and tree["defined"] == want["defined"], what
    if want["defined"] == 0:
        assert np.isnan(stats[2:]).all() and np.isnan(tree["mean"]) and np.isnan(tree["max"]), what
        return
    assert np.float64(stats[3]).view(np.uint64) == np.float64(want["max"]).view(np.uint64), "%s: largest %r != %r" % (what, stats[3], want["max"])
    bound = 2.0 * want["defined"] * 2.0 ** -53
    rel = abs(stats[2] - want["mean"]) / want["mean"] if want["mean"] else abs(stats[2])
    print("%s: kept %d of %d defined, mean off by %.3g relative (bound %.3g); mean %.17g, the documented tree's %.17g"
          % (what, want["kept"], want["defined"], rel, bound, stats[2], tree["mean"]))
    assert rel <= bound, what
    assert rt.bits(stats[3]) == rt.bits(tree["max"]), "%s: largest %r, the tree's %r" % (what, stats[3], tree["max"])
    assert rt.bits(stats[2]) == rt.bits(tree["mean"]), "%s: the mean %.17g is not that of the documented order, %.17g" % (what, stats[2], tree["mean"])
