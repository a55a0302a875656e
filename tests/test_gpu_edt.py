"""GPU: the exact Euclidean distance transform (csrc/pdeip_edt.hip) and what stands on it, bit for bit against the NumPy restatement
(tests/edt_ref.py) on the cases of tests/edt_cases.py:

  d2, idx and dist for every mask, mode and max_dist; frames; every combination of missing outputs; the host entry point
  bwdist, signed_distance and nearest_fill through device.*, drivers.* and the MEX stub; inputs unchanged; out == D for the fill
  planes at a 4-byte offset; the stated launch counts; a graph capture replayed twice
  the interpolation chain with the nearest-source fill through device, drivers and interpolate_frames; the unchanged default
  GAC_v10a started from the signed distance of its initial mask"""
import importlib

import numpy as np
import pytest

import edt_cases as ec
import edt_ref
import interp_cases as ic
import problems as pb

pytestmark = pytest.mark.gpu
F32, F64, I32 = np.float32, np.float64, np.int32
SUBSET = [((1, 1), "full"), ((1, 1), "empty"), ((1, 70), "rand5"), ((70, 1), "pair"), ((3, 3), "centre"), ((5, 90), "quad"), ((131, 6), "diagonal"),
          ((37, 53), "splat"), ((37, 53), "empty"), ((37, 53), "full"), ((64, 64), "checker"), ((65, 257), "rand05"), ((65, 257), "rand50")]


def sub(name):
    return importlib.import_module("pde-based-image-processing_amd." + name)


def same(got, want, what):
    assert pb.bit_equal(got, want), "%s: %s" % (what, pb.describe_mismatch(got, want))


def same_int(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == I32 and got.shape == want.shape, what
    assert np.array_equal(got, want), "%s: %s" % (what, pb.describe_mismatch(got, want))


def up(a):
    """A case on the device (the cases are read-only; torch wants a writable array to wrap)."""
    return sub("device").to_device(np.array(a, dtype=F32, order="F"))


def down(t):
    return None if t is None else sub("device").to_matlab(t)


def carve(t):
    """The same values in a tensor that starts 4 bytes into its allocation."""
    import torch

    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = flat[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 8 == 4 and out.is_contiguous()
    return out


def launches(pdeip):
    return pdeip.capi.load().pdeip_last_launch_count()


def bits(t):
    return t.cpu().numpy().tobytes()


def check_edt(got, want, what):
    same_int(got[0], want[0], what + " d2")
    same_int(got[1], want[1], what + " idx")
    same(got[2], want[2], what + " dist")


# ---- the transform -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ec.SMALL_SHAPES, ids=ec.shape_id)
def test_transform(pdeip, shape):
    """Every mask kind of a shape (one test per shape: the cases are small and many): every predicate on its own dressing of the
    mask, the complement through the _NOT twin, every max_dist."""
    for case in ec.cases():
        if case[0] == shape:
            _check_transform(case)


def _check_transform(case):
    dev = sub("device")
    shape, kind = case
    for base in ec.BASE_MODES:
        tA = up(ec.plane(shape, kind, base))
        before = bits(tA)
        for complement in (False, True):
            mode = base | (4 if complement else 0)
            for R in ec.MAX_DISTS:
                got = [down(t) for t in dev.edt(tA, edt_ref.MODE_NAMES[mode], R)]
                check_edt(got, ec.want(shape, kind, complement, R), "%s mode %d max_dist %d" % (ec.case_id(case), mode, R))
        assert bits(tA) == before, "the input was modified"


def test_many_workgroups_once(pdeip):
    """270 x 480, 5 % features: many workgroups per column pass and row pass, through the device form and the host entry point."""
    dev = sub("device")
    M = ec.mask(ec.BIG_SHAPE, "rand5")
    A = np.asfortranarray(np.where(M, F32(2.0), F32(np.nan)))
    for R in (0, 3):
        want = edt_ref.edt(A, edt_ref.POSITIVE, R)
        check_edt([down(t) for t in dev.edt(up(A), "positive", R)], want, "big max_dist %d" % R)
        d2, idx, dist = np.zeros(A.shape, I32, order="F"), np.zeros(A.shape, I32, order="F"), np.zeros(A.shape, F32, order="F")
        pdeip.capi.call("pdeip_edt", A.ctypes.data, A.shape[0], A.shape[1], 1, edt_ref.POSITIVE, R, d2.ctypes.data, idx.ctypes.data,
                        dist.ctypes.data)
        check_edt((d2, idx, dist), want, "big, host pointers, max_dist %d" % R)


def test_frames_are_transformed_on_their_own(pdeip):
    for fc in ec.FRAME_CASES:
        _check_frames(pdeip, fc)


def _check_frames(pdeip, fc):
    dev = sub("device")
    shape, kinds = fc
    for base in (edt_ref.POSITIVE, edt_ref.NOT_NAN):
        A = ec.frames(shape, kinds, base)
        for complement, R in ((False, 0), (True, 3)):
            got = [down(t) for t in dev.edt(up(A), base | (4 if complement else 0), R)]
            check_edt(got, ec.want_frames(shape, kinds, complement, R), "frames %s mode %d" % (ec.shape_id(shape), base))
    A = np.array(ec.frames(shape, kinds, edt_ref.NONNEG), order="F")
    d2, idx, dist = np.zeros(A.shape, I32, order="F"), np.zeros(A.shape, I32, order="F"), np.zeros(A.shape, F32, order="F")
    pdeip.capi.call("pdeip_edt", A.ctypes.data, shape[0], shape[1], len(kinds), edt_ref.NONNEG, 0, d2.ctypes.data, idx.ctypes.data,
                    dist.ctypes.data)
    check_edt((d2, idx, dist), ec.want_frames(shape, kinds, False, 0), "frames, host pointers")


def test_any_output_may_be_missing(pdeip):
    import torch

    dev = sub("device")
    shape, kind = (37, 53), "rand5"
    tA = up(ec.plane(shape, kind, edt_ref.POSITIVE))
    want = ec.want(shape, kind, False, 3)
    for pick in range(1, 8):
        flags = [bool(pick & 1), bool(pick & 2), bool(pick & 4)]
        got = dev.edt(tA, "positive", 3, d2=flags[0], idx=flags[1], dist=flags[2])
        for k, name in enumerate(("d2", "idx", "dist")):
            if not flags[k]:
                assert got[k] is None
            elif k < 2:
                same_int(down(got[k]), want[k], "outputs %s: %s" % (flags, name))
            else:
                same(down(got[k]), want[k], "outputs %s: dist" % flags)
    with pytest.raises(pdeip.capi.PdeipError, match="all NULL"):
        dev.edt(tA, "positive", 3, d2=False, idx=False, dist=False)
    D, IDX = dev.bwdist(tA, idx=False)
    assert IDX is None
    same(down(D), ec.want(shape, kind, False, 0)[2], "bwdist without IDX")
    idx_only = torch.zeros(tA.shape, dtype=torch.int32, device=tA.device)
    pdeip.capi.call("pdeip_bwdist_dev", dev._stream(), tA.data_ptr(), shape[0], shape[1], 1, None, idx_only.data_ptr())
    same_int(down(idx_only), ec.want(shape, kind, False, 0)[1], "bwdist without D")


# ---- bwdist, signed distance, nearest fill ---------------------------------------------------------------------------------------------

def test_bwdist(pdeip):
    for case in SUBSET:
        _check_bwdist(pdeip, case)


def _check_bwdist(pdeip, case):
    from test_edt_stub import OUT, build_morph_stub
    from test_flowviz_stub import call_typed

    dev, drv = sub("device"), sub("drivers")
    shape, kind = case
    A = np.array(ec.plane(shape, kind, edt_ref.POSITIVE), order="F")
    _, widx, wdist = ec.want(shape, kind, False, 0)
    tA = up(A)
    before = bits(tA)
    D, IDX = dev.bwdist(tA)
    assert launches(pdeip) == 2
    same(down(D), wdist, "device.bwdist D")
    same_int(down(IDX), widx, "device.bwdist IDX")
    assert bits(tA) == before
    for BW in (ec.mask(shape, kind), A):                   # a logical mask, and numbers of which the positive ones count
        D, IDX = drv.bwdist(BW)
        same(D, wdist, "drivers.bwdist D")
        same_int(IDX, widx, "drivers.bwdist IDX")
    lib = build_morph_stub("bwdist_gpu", pdeip)
    for arg in (A, A.astype(F64)):
        err, outs = call_typed(lib, OUT, [arg])
        assert err is None, err
        same(outs[0], wdist, "stub D")
        assert np.array_equal(outs[1].view(np.uint32), (widx.astype(np.int64) + 1).astype(np.uint32)), "stub IDX: 1-based, 0 = none"
    err, outs = call_typed(lib, (F32,), [A])
    assert err is None and outs[0].tobytes(order="F") == np.asarray(wdist).tobytes(order="F")


def test_signed_distance(pdeip):
    for case in SUBSET:
        _check_signed_distance(pdeip, case)
    _check_signed_distance_of_frames(pdeip)


def _check_signed_distance(pdeip, case):
    dev, drv = sub("device"), sub("drivers")
    shape, kind = case
    A = ec.plane(shape, kind, edt_ref.NONNEG)
    for R in (0, 3):
        want = edt_ref.signed_distance(A, R)
        tA = up(A)
        before = bits(tA)
        same(down(dev.signed_distance(tA, R)), want, "device.signed_distance max_dist %d" % R)
        assert launches(pdeip) == 5 and bits(tA) == before
        same(drv.signed_distance(A, R), want, "drivers.signed_distance max_dist %d" % R)
        assert dev.signed_distance(tA, R, out=tA) is tA
        same(down(tA), want, "signed_distance in place")
        if kind not in ("full", "empty") or R:
            assert np.isfinite(want).all() and (np.abs(want) >= 0.5).all()
    if kind in ("full", "empty"):
        assert (edt_ref.signed_distance(A, 0) == (np.inf if kind == "full" else -np.inf)).all()


def _check_signed_distance_of_frames(pdeip):
    shape, kinds = ec.FRAME_CASES[0]
    A = ec.frames(shape, kinds, edt_ref.NONNEG)
    want = edt_ref.signed_distance(A, 0)
    same(down(sub("device").signed_distance(up(A))), want, "device.signed_distance, 3 frames")
    same(sub("drivers").signed_distance(A), want, "drivers.signed_distance, 3 frames")


def test_nearest_fill(pdeip):
    for case in SUBSET:
        _check_nearest_fill(pdeip, case)
    _check_nearest_fill_of_frames(pdeip)


def _check_nearest_fill(pdeip, case):
    import torch

    dev, drv = sub("device"), sub("drivers")
    shape, kind = case
    D = ec.sparse_map(shape, kind)
    for R in (0, 3):
        want = edt_ref.nearest_fill(D, R)
        what = "%s max_dist %d " % (ec.case_id(case), R)
        tD = up(D)
        before = bits(tD)
        filled, dist = torch.full_like(tD, 7), torch.full_like(tD, 7)
        out = dev.nearest_fill(tD, R, filled_out=filled, dist_out=dist)
        assert launches(pdeip) == 3 and bits(tD) == before, "launches / the input was modified"
        for g, w, name in zip((out, filled, dist), want, ("out", "filled", "dist")):
            same(down(g), w, what + "device " + name)
        got = drv.nearest_fill(D, R, return_filled=True, return_dist=True)
        for g, w, name in zip(got, want, ("out", "filled", "dist")):
            same(g, w, what + "drivers " + name)
        same(drv.nearest_fill(D, R), want[0], what + "drivers, out alone")
        assert dev.nearest_fill(tD, R, out=tD) is tD                  # out == D: known pixels are not stored, holes are not read
        same(down(tD), want[0], what + "in place")
    known = ~np.isnan(D)
    assert np.array_equal(edt_ref.nearest_fill(D, 0)[0][known].view(np.uint32), np.asarray(D)[known].view(np.uint32))


def _check_nearest_fill_of_frames(pdeip):
    shape, kinds = ec.FRAME_CASES[0]
    D = np.asfortranarray(np.stack([ec.sparse_map(shape, k) for k in kinds], axis=2))
    want = edt_ref.nearest_fill(D, 0)
    assert np.isnan(want[0][:, :, 1]).all(), "the empty frame stays NaN"
    same(down(sub("device").nearest_fill(up(D))), want[0], "device.nearest_fill, 3 frames")
    got = sub("drivers").nearest_fill(D, return_filled=True)
    same(got[0], want[0], "drivers.nearest_fill, 3 frames")
    same(got[1], want[1], "drivers.nearest_fill, 3 frames, filled")


def test_planes_at_a_4_byte_offset(pdeip):
    import torch

    dev = sub("device")
    shape, kind = (65, 257), "rand5"
    tA = carve(up(ec.plane(shape, kind, edt_ref.POSITIVE)))
    outs = [carve(torch.zeros(tA.shape, dtype=t, device=tA.device)) for t in (torch.int32, torch.int32, torch.float32)]
    dev.edt(tA, "positive", 0, d2_out=outs[0], idx_out=outs[1], dist_out=outs[2])
    check_edt([down(t) for t in outs], ec.want(shape, kind, False, 0), "carved edt")
    tN = carve(up(ec.plane(shape, kind, edt_ref.NONNEG)))
    same(down(dev.signed_distance(tN, 0, out=carve(torch.zeros_like(tN)))), edt_ref.signed_distance(ec.plane(shape, kind, edt_ref.NONNEG)),
         "carved signed_distance")
    D = ec.sparse_map(shape, kind)
    want = edt_ref.nearest_fill(D, 0)
    tD = carve(up(D))
    filled = carve(torch.zeros_like(tD))
    same(down(dev.nearest_fill(tD, 0, out=carve(torch.zeros_like(tD)), filled_out=filled)), want[0], "carved nearest_fill")
    same(down(filled), want[1], "carved nearest_fill filled")


# ---- launch counts and graph capture -------------------------------------------------------------------------------------------------

def scene_tensors():
    return [up(np.array(a, order="F")) for a in ic.scene()[:7]]


def test_launch_counts_do_not_depend_on_the_data(pdeip):
    import torch

    dev = sub("device")
    for shape in ((1, 1), (37, 53), (300, 70)):
        for fill in (1.0, float("nan"), -1.0):
            t = torch.full((shape[1], shape[0]), fill, dtype=torch.float32, device="cuda")
            for mode in edt_ref.MODES:
                dev.edt(t, mode, 2)
                assert launches(pdeip) == 2
            dev.bwdist(t)
            assert launches(pdeip) == 2
            dev.signed_distance(t)
            assert launches(pdeip) == 5
            dev.nearest_fill(t)
            assert launches(pdeip) == 3
    tI0, tI1, _, tUf, tVf, tUb, tVb = scene_tensors()
    nan = torch.full_like(tUf, float("nan"))
    kw = dict(fill_with="nearest")
    dev.flow_interpolate(tI0, tI1, tUf, tVf, tUb, tVb, **kw)
    assert launches(pdeip) == 2 + 3 + 2 + 1 + 1 + 2, "cross-checks, splat, transform, gather, blend, two copies"
    dev.flow_interpolate(tI0, tI1, tUf, tVf, **kw)
    assert launches(pdeip) == 3 + 2 + 1 + 1 + 2
    dev.flow_interpolate(tI0, tI1, tUf, tVf, tUb, tVb, flow=False, source=False, max_dist=2, **kw)
    assert launches(pdeip) == 2 + 3 + 2 + 1 + 1
    dev.flow_interpolate(tI0, tI1, nan, tVf, tUb, nan, flow=False, use_costs=0, **kw)      # no source, no consistent pixel
    assert launches(pdeip) == 2 + 3 + 2 + 1 + 1, "the count must not depend on the data"
    torch.cuda.synchronize()


def test_captured_in_a_graph(pdeip):
    """The transform, the signed distance, the fill and the chain captured on a side stream after eager calls have created the
    workspaces; replayed twice on changed inputs with every output filled beforehand, each replay equals the eager calls bit for bit."""
    import torch

    dev = sub("device")
    tI0, tI1, _, tUf, tVf, tUb, tVb = scene_tensors()
    shape = ic.SCENE_SHAPE
    tA = up(ec.sparse_map((37, 53), "rand5"))

    def new():
        like = lambda t, dt=torch.float32: torch.zeros(t.shape, dtype=dt, device=t.device)
        return dict(d2=like(tA, torch.int32), idx=like(tA, torch.int32), dist=like(tA), sdf=like(tA), fill=like(tA), filled=like(tA),
                    It=like(tI0), Ut=like(tUf), Vt=like(tUf), src=like(tUf))

    def enqueue(o):
        dev.edt(tA, "not_nan", 0, d2_out=o["d2"], idx_out=o["idx"], dist_out=o["dist"])
        dev.signed_distance(tA, 4, out=o["sdf"])
        dev.nearest_fill(tA, 0, out=o["fill"], filled_out=o["filled"])
        dev.flow_interpolate(tI0, tI1, tUf, tVf, tUb, tVb, t=0.5, It_out=o["It"], Ut_out=o["Ut"], Vt_out=o["Vt"], source_out=o["src"],
                             fill_with="nearest")

    cap = new()
    enqueue(cap)    # the workspaces exist before the capture
    torch.cuda.synchronize()
    generation = pdeip.capi.load().pdeip_workspace_generation()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        enqueue(cap)
    torch.cuda.current_stream().wait_stream(side)
    assert pdeip.capi.load().pdeip_workspace_generation() == generation, "the capture must not touch the workspaces"
    moved = np.array(ic.scene()[3])
    moved[40:60, 20:90] = -3.5
    moved[::9, ::7] = np.nan
    for U, other in ((moved, ec.sparse_map((37, 53), "checker")), (np.array(ic.scene()[3]), ec.sparse_map((37, 53), "rand5"))):
        tUf.copy_(up(U))
        tA.copy_(up(other))
        for t in cap.values():
            t.fill_(7)      # the replay must write everything
        graph.replay()
        torch.cuda.synchronize()
        eager = new()
        enqueue(eager)
        torch.cuda.synchronize()
        for k in cap:
            assert bits(cap[k]) == bits(eager[k]), "replay differs from the eager call in " + k
        same(down(cap["fill"]), edt_ref.nearest_fill(other, 0)[0], "replayed fill against the restatement")
    assert shape == tuple(reversed(tUf.shape))


# ---- the interpolation chain -----------------------------------------------------------------------------------------------------------

def test_chain_on_the_scene(pdeip):
    for backward in (False, True):
        _check_chain_on_the_scene(backward)


def _check_chain_on_the_scene(backward):
    dev, drv = sub("device"), sub("drivers")
    I0, I1, Imid, Uf, Vf, Ub, Vb = [np.array(a, order="F") for a in ic.scene()[:7]]
    back = (Ub, Vb) if backward else (None, None)
    for R in (0, 2):
        want = edt_ref.flow_interpolate_nearest(I0, I1, Uf, Vf, back[0], back[1], t=0.5, max_dist=R)
        what = "scene backward %s max_dist %d: " % (backward, R)
        a = drv.flow_interpolate(I0, I1, Uf, Vf, back[0], back[1], t=0.5, return_flow=True, return_source=True, fill_with="nearest", max_dist=R)
        a = (a[0], a[1][:, :, 0], a[1][:, :, 1], a[2])
        tin = [up(x) for x in (I0, I1, Uf, Vf)] + [None if x is None else up(x) for x in back]
        before = [None if x is None else bits(x) for x in tin]
        b = dev.flow_interpolate(*tin, t=0.5, fill_with="nearest", max_dist=R)
        assert [None if x is None else bits(x) for x in tin] == before, "an input was modified"
        b = [down(x) for x in b]
        for k, name in enumerate(("It", "Ut", "Vt", "source")):
            for got, who in ((a[k], "drivers"), (b[k], "device")):
                same(np.asarray(got).reshape(want[k].shape, order="F"), want[k], what + who + " " + name)
        only = drv.flow_interpolate(I0, I1, Uf, Vf, back[0], back[1], t=0.5, fill_with="nearest", max_dist=R)
        assert np.asarray(only).tobytes(order="F") == np.asarray(a[0]).tobytes(order="F")
        if R == 0:
            valid = ic.scene()[7]
            assert np.isfinite(want[1]).all()
            print(what + "RMS against the true middle frame %.4f (average of the frames %.4f)"
                  % (ic.rms(want[0], Imid, valid), ic.rms((I0.astype(F64) + I1.astype(F64)) / 2, Imid, valid)))


def test_a_colour_pair_with_holes_and_a_field_without_a_source(pdeip):
    dev = sub("device")
    shape = (37, 53)
    Uf, Vf, I0, I1 = ic.field(shape, "expand")           # three channels; the expansion leaves a grid of holes
    Ub, Vb = np.asfortranarray(-Uf), np.asfortranarray(-Vf)
    want = edt_ref.flow_interpolate_nearest(I0, I1, Uf, Vf, Ub, Vb, t=0.25, a=0.0, b=2.0, use_costs=0)
    got = dev.flow_interpolate(up(I0), up(I1), up(Uf), up(Vf), up(Ub), up(Vb), t=0.25, a=0.0, b=2.0, use_costs=0, fill_with="nearest")
    for g, w, name in zip(got, want, ("It", "Ut", "Vt", "source")):
        same(down(g), w, "colour pair " + name)
    Uf, Vf, I0, I1 = ic.field(shape, "all_nonfinite")    # every pixel a hole without a source: zeros, hence the zero-flow blend
    It, Ut, Vt, src = dev.flow_interpolate(up(I0), up(I1), up(Uf), up(Vf), t=0.25, fill_with="nearest")
    assert (down(Ut).view(np.uint32) == 0).all() and (down(Vt).view(np.uint32) == 0).all()
    same(down(It), (0.75 * I0.astype(F64) + 0.25 * I1.astype(F64)).astype(F32), "all holes")
    assert (down(src) == 3).all()


def test_the_default_is_unchanged(pdeip):
    """No new keyword, and fill_with="tv" spelled out, go down the existing path: identical bytes, and the TV chain's launch count."""
    dev, drv = sub("device"), sub("drivers")
    I0, I1, Imid, Uf, Vf, Ub, Vb = [np.array(a, order="F") for a in ic.scene()[:7]]
    prm = dict(outer_iter=2, mode=1)
    a = drv.flow_interpolate(I0, I1, Uf, Vf, Ub, Vb, t=0.5, return_flow=True, return_source=True, **prm)
    b = drv.flow_interpolate(I0, I1, Uf, Vf, Ub, Vb, t=0.5, return_flow=True, return_source=True, fill_with="tv", **prm)
    for x, y in zip(a, b):
        assert x.tobytes(order="F") == y.tobytes(order="F")
    tin = [up(x) for x in (I0, I1, Uf, Vf, Ub, Vb)]
    c = dev.flow_interpolate(*tin, t=0.5, **prm)
    n = launches(pdeip)
    d = dev.flow_interpolate(*tin, t=0.5, fill_with="tv", **prm)
    assert launches(pdeip) == n > 2 + 3 + 2 + 1 + 1 + 2
    for x, y in zip(c, d):
        assert bits(x) == bits(y)
    assert a[0].tobytes(order="F") == down(c[0]).reshape(a[0].shape, order="F").tobytes(order="F")
    near = drv.flow_interpolate(I0, I1, Uf, Vf, Ub, Vb, t=0.5, fill_with="nearest")
    assert near.tobytes(order="F") != a[0].tobytes(order="F"), "the two fills are different fills"
    sub("device").sync_check()


def test_interpolate_frames_with_the_nearest_fill(pdeip):
    """A 60 x 80 textured pair, the second frame the first moved 2 px to the right: interpolate_frames hands fill_with through its
    interp=dict(...), and its frame is flow_interpolate's on the same flows, which is the restatement's."""
    drv = sub("drivers")
    rng = np.random.default_rng(5)
    base = rng.random((60, 120))
    for _ in range(6):      # a few passes of a 3 x 3 box: texture a flow can be computed on
        base = (base + np.roll(base, 1, 0) + np.roll(base, -1, 0)) / 3
        base = (base + np.roll(base, 1, 1) + np.roll(base, -1, 1)) / 3
    base = ((base - base.min()) / (base.max() - base.min()) * 255).astype(F32)
    I0, I1 = np.asfortranarray(base[:, 20:100]), np.asfortranarray(base[:, 18:98])
    Iin = np.stack([I0, I1], axis=2)
    frames, fwd, bwd = drv.interpolate_frames(Iin, 1, t=(0.5,), return_flows=True, interp=dict(fill_with="nearest", max_dist=8))
    assert len(frames) == 1 and frames[0].shape == (60, 80) and frames[0].dtype == F32
    flows = [np.asfortranarray(f[:, :, k]) for f in (fwd, bwd) for k in (0, 1)]
    alone = drv.flow_interpolate(I0, I1, *flows, t=0.5, fill_with="nearest", max_dist=8)
    same(alone, frames[0], "interpolate_frames against flow_interpolate on its flows")
    want = edt_ref.flow_interpolate_nearest(I0, I1, *flows, t=0.5, max_dist=8)
    same(frames[0], want[0], "interpolate_frames against the restatement")


# ---- a level set started from its signed distance ------------------------------------------------------------------------------------

def test_gac_from_the_signed_distance(pdeip):
    """GAC_v10a(I, signed_distance(PHI)) on the drivsco image with runme.m's box: the driver is untouched, so its result is the
    restated driver's on the restated signed distance, bit for bit."""
    import levelset_ref
    from test_gpu_levelset import _drivsco

    drv = sub("drivers")
    imgs, PHI = _drivsco()
    S = drv.signed_distance(PHI)
    want_S = edt_ref.signed_distance(PHI)
    same(S, want_S, "signed distance of the initial box")
    assert np.isfinite(S).all() and S.max() > 40 and S.min() < -40, "a distance function, not a band"
    got = drv.GAC_v10a(imgs[0], S, ITER=5)
    want = levelset_ref.GAC(imgs[0], want_S, "a", ITER=5)
    same(got, want, "GAC_v10a from the signed distance")
    assert not pb.bit_equal(got, drv.GAC_v10a(imgs[0], PHI, ITER=5)), "the start matters"
