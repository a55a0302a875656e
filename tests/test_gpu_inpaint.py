"""GPU: the hole filling (csrc/pdeip_inpaint.hip) against its restatement (inpaint_ref.py, pinned by test_inpaint_ref.py) on the seeded
cases of inpaint_cases.py.  Everything is bit for bit with any NaN equal to any NaN (problems.bit_equal): the stage kernels are
correctly rounded IEEE operations in the restatement's order, the solver between them is the library's PDEsolver4, bit-exact against
the oracle in both orderings.

  nan_resize, inpaint_meanfill, tv4_inpaint_assemble, inpaint_merge   each against the restatement; one launch each
  Inpaint4Level                                                       one 56 x 72 level against the restatement, four (solver, mode) pairs
  drivers.TVinpaint4, drivers.capi_TVinpaint4, device.tv_inpaint4     the 96 x 128 scene: equal among themselves and to the restatement
  launch counts, graph replay, stereo_maps(fill=True), the MEX stub
"""
import functools
import importlib

import numpy as np
import pytest

import inpaint_cases as ic
import inpaint_ref as ir
import problems as pb

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64


def sub(name):
    return importlib.import_module("pde-based-image-processing_amd." + name)


def same(got, want, what):
    assert pb.bit_equal(got, want), "%s: %s" % (what, pb.describe_mismatch(got, want))


def up(a):
    """A case on the device (the cases are read-only; torch wants a writable array to wrap)."""
    return sub("device").to_device(np.array(a, dtype=F32, order="F"))


def launches(pdeip):
    return pdeip.capi.load().pdeip_last_launch_count()


def writable_scene():
    """The scene as arrays of the caller's own (the drivers wrap their inputs for torch, which wants writable memory)."""
    truth, sparse, guide, band = ic.scene()
    return np.array(truth, order="F"), np.array(sparse, order="F"), np.array(guide, order="F"), band


def stage_planes():
    """(name, sparse map) of the resize / fill tests: every shape with every hole pattern, and the tie plane."""
    for shape, out in ic.RESIZE_SHAPES:
        for kind in ic.HOLE_KINDS:
            yield "%dx%d %s" % (shape + (kind,)), ic.holed(shape, kind), out
    yield "tie", ic.tie_plane(), (4, 4)


# ---- the stage kernels ---------------------------------------------------------------------------------------------------------------

def test_nan_resize(pdeip):
    dev = sub("device")
    for name, D, out in stage_planes():
        for cover in (0.25, 0.5, 1.0):
            got = dev.nan_resize(up(D), out[0], out[1], cover)
            assert launches(pdeip) == 1
            want = ir.nan_resize(D, out[0], out[1], cover)
            same(dev.to_matlab(got), want, "nan_resize %s cover %g" % (name, cover))
    kept = dev.to_matlab(dev.nan_resize(up(ic.tie_plane()), 4, 4, 0.5))
    assert not np.isnan(kept).any(), "den == cover must keep the pixel"
    assert np.isnan(dev.to_matlab(dev.nan_resize(up(ic.tie_plane()), 4, 4, float(np.nextafter(0.5, 1.0))))).all()
    full = ic.holed((37, 53), "none")
    same(dev.to_matlab(dev.nan_resize(up(full), 28, 40, 1e-9)), dev.to_matlab(dev.pyr_resize(up(full), 28, 40)), "known plane: pyr_resize")


def test_inpaint_meanfill(pdeip):
    dev = sub("device")
    cases = [(name, D) for name, D, _ in stage_planes()]
    cases += [("single known %dx%d" % s, ic.single_known(s)) for s in ((37, 53), (5, 90), (131, 6))]
    cases.append(("wide 3x700", ic.holed((3, 700), "random")))    # more columns than one round of the workgroup sums
    for name, D in cases:
        t = up(D)
        got = dev.inpaint_meanfill(t)
        assert launches(pdeip) == 1
        want = ir.meanfill(D)
        same(dev.to_matlab(got), want, "meanfill " + name)
        assert not np.isnan(want).any()
        assert dev.to_matlab(t).tobytes() == np.asfortranarray(D).tobytes(), "the input was modified"
        same(dev.to_matlab(dev.inpaint_meanfill(t, out=t)), want, "meanfill in place " + name)


@pytest.mark.parametrize("holes", ic.ASSEMBLE_HOLES)
@pytest.mark.parametrize("shape,F,G", ic.ASSEMBLE_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_tv4_inpaint_assemble(pdeip, shape, F, G, holes):
    import torch

    dev = sub("device")
    X, D, guide = ic.assemble_case(shape, F, G, holes)
    tX, tD, tG = up(X), up(D), None if guide is None else up(guide)
    TRACE, B = torch.full_like(tX, 3.0), torch.full_like(tX, 3.0)
    w4 = [torch.full_like(tX, 3.0) for _ in range(4)]
    dev.tv4_inpaint_assemble(tX, tD, 5.0, TRACE, B, w4, tG, 20.0)
    assert launches(pdeip) == 1
    wT, wB, ww = ir.assemble(X, D, 5.0, guide, 20.0)
    what = "assemble %s F %d G %d %s" % (shape, F, G, holes)
    hole = np.isnan(D)
    gT, gB = dev.to_matlab(TRACE), dev.to_matlab(B)
    same(gT, wT, what + " TRACE")
    assert np.array_equal(np.isnan(gT), hole)
    same(gB, wB, what + " B")
    assert (gB[hole].view(np.uint32) == 0).all(), "B must be exactly +0 on holes"
    for k, (g, w) in enumerate(zip(w4, ww)):
        same(dev.to_matlab(g), w, what + " weight %d" % k)
    if holes == "none" and G == 0:   # the denoiser's own assembly, bit for bit
        T2, B2 = torch.empty_like(tX), torch.empty_like(tX)
        v4 = [torch.empty_like(tX) for _ in range(4)]
        dev.tv4_assemble(tX, tD, 5.0, T2, B2, v4)
        for a, b in zip([TRACE, B] + w4, [T2, B2] + v4):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_inpaint_merge(pdeip):
    import torch

    dev = sub("device")
    D = np.asfortranarray(ic.smooth_plane((37, 53), 41, frames=2))
    rng = np.random.default_rng(43)
    D[rng.random(D.shape) < 0.3] = np.nan
    D[0, 0, 0], D[1, 0, 0], D[2, 0, 0], D[3, 0, 1], D[36, 52, 1] = -0.0, np.inf, -np.inf, 1e-45, np.nan
    X = ic.smooth_plane((37, 53), 47, frames=2)
    want, wfilled = ir.merge(X, D)
    tX, tD = up(X), up(D)
    got = dev.inpaint_merge(tX, tD)                       # filled_out NULL
    assert launches(pdeip) == 1
    filled = torch.full_like(tX, 5.0)
    got2 = dev.inpaint_merge(tX, tD, filled_out=filled)
    assert launches(pdeip) == 1
    for g in (got, got2):
        g = dev.to_matlab(g)
        same(g, want, "merge")
        known = ~np.isnan(D)
        assert g[known].tobytes() == D[known].tobytes() and np.signbit(g[0, 0, 0]) and g[1, 0, 0] == np.inf
    assert np.array_equal(dev.to_matlab(filled), wfilled) and np.array_equal(wfilled, np.isnan(D).astype(F32))
    inplace = up(X)
    dev.inpaint_merge(inplace, tD, out=inplace)
    same(dev.to_matlab(inplace), want, "merge into X")


# ---- one level -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("solver,mode,order,F,guided", [(1, 0, 0, 1, False), (1, 1, 1, 2, False), (2, 0, 0, 2, False), (2, 1, 1, 1, False),
                                                        (2, 0, 0, 1, True), (1, 1, 1, 2, True)])
def test_inpaint4_level(pdeip, oracle, solver, mode, order, F, guided):
    dev = sub("device")
    D, X0, guide = ic.level_case(F, guided)
    hole = np.isnan(D)
    assert 0.18 < hole.mean() < 0.26
    param = dict(alpha=5.0, omega=1.75, outer_iter=3, inner_iter=5, solver=solver, order=order, guide_scale=20.0)
    want = ir.level(oracle, D, X0, param, guide)
    got = sub("flow_level").Inpaint4Level(param, mode=mode).run(up(D), up(X0), None if guide is None else up(guide))
    same(dev.to_matlab(got), want, "inpaint level (solver %d mode %d F %d guide %s)" % (solver, mode, F, guided))
    assert np.isfinite(want).all()


# ---- the driver ----------------------------------------------------------------------------------------------------------------------

SCENE_PARAM = dict(outer_iter=3)


@functools.lru_cache(maxsize=None)
def scene_want(guided, order):
    import oracle_lib

    oracle_lib.lib()
    truth, sparse, guide, band = ic.scene()
    X, filled = ir.tv_inpaint4(oracle_lib, sparse, guide if guided else None, keep=0, order=order, **SCENE_PARAM)
    return X, ir.merge(X, sparse)[0], filled


@pytest.mark.parametrize("mode", [0, 1], ids=["exact_order", "red_black"])
@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
def test_driver_on_the_scene(pdeip, guided, mode):
    dev, drv = sub("device"), sub("drivers")
    truth, sparse, guide, band = writable_scene()
    g = guide if guided else None
    raw, merged, wfilled = scene_want(guided, mode)
    hole = np.isnan(sparse)
    assert np.array_equal(wfilled, hole.astype(F32))
    for keep, want in ((1, merged), (0, raw)):
        what = "scene guided %s mode %d keep %d: " % (guided, mode, keep)
        a, fa = drv.TVinpaint4(sparse, guide=g, mode=mode, return_filled=True, keep=keep, **SCENE_PARAM)
        b, fb = drv.capi_TVinpaint4(sparse, guide=g, mode=mode, return_filled=True, keep=keep, **SCENE_PARAM)
        tf = up(np.full(sparse.shape, 5.0, F32))
        c = dev.to_matlab(dev.tv_inpaint4(up(sparse), None if g is None else up(g), filled_out=tf, mode=mode, keep=keep, **SCENE_PARAM))
        assert pdeip.capi.last_error() == ""
        same(a, want, what + "TVinpaint4")
        same(b, want, what + "capi_TVinpaint4")
        same(c, want, what + "device.tv_inpaint4")
        for f in (fa, fb, dev.to_matlab(tf)):
            assert np.array_equal(f, wfilled), what + "filled"
        assert np.isfinite(a).all()
        if keep:
            assert a[~hole].tobytes() == sparse[~hole].tobytes(), what + "known pixels must come back with their own bits"
        assert np.asarray(drv.TVinpaint4(sparse, guide=g, mode=mode, keep=keep, **SCENE_PARAM)).tobytes() == a.tobytes()
    if mode == 0:
        print("scene, outer_iter 3, guided %s: RMS over the holes %.3f px (mean fill %.3f)"
              % (guided, ic.rms(merged, truth, hole), ic.rms(ir.meanfill(sparse), truth, hole)))


def test_a_flow_is_two_frames(pdeip, oracle):
    """U, V as two frames with joint weights, through the three entry points."""
    dev, drv = sub("device"), sub("drivers")
    D = np.array(ic.holed((37, 53), "empty_frame"))
    D[:, :, 0] = ic.holed((37, 53), "random")
    D[10:20, 30:39, 1] = np.nan
    p = dict(outer_iter=2, min_size=8)
    want, wfilled = ir.tv_inpaint4(oracle, D, order=1, **p)
    a, fa = drv.TVinpaint4(D, mode=1, return_filled=True, **p)
    b = drv.capi_TVinpaint4(D, mode=1, **p)
    c = dev.to_matlab(dev.tv_inpaint4(up(D), mode=1, **p))
    for got in (a, b, c):
        same(got, want, "two frames")
    assert np.array_equal(fa, wfilled)


def test_launch_counts_do_not_depend_on_the_data(pdeip):
    dev = sub("device")
    truth, sparse, guide, band = ic.scene()
    half = np.array(truth)
    half[:, 64:] = np.nan
    counts = {}
    for mode in (0, 1):
        for solver in (1, 2):
            for name, D in (("known", truth), ("scene", sparse), ("half", half)):
                dev.tv_inpaint4(up(D), up(guide), mode=mode, solver=solver, **SCENE_PARAM)
                counts[(mode, solver, name)] = launches(pdeip)
            assert counts[(mode, solver, "known")] == counts[(mode, solver, "scene")] == counts[(mode, solver, "half")] > 0, counts
    dev.sync_check()
    # 7 levels: 6 + 6 resizes, 1 fill, 6 resizes up, 1 merge, and per level 4 x (1 assembly + the solver's launches)
    assert len(ir.sizes(96, 128, 0.75, 16)) == 7
    assert all(n >= 20 + 7 * 4 * 2 for n in counts.values()), counts
    print("launches of the driver on 96x128, outer_iter 3, guide: %r" % {k[:2]: v for k, v in counts.items() if k[2] == "known"})


def test_captured_in_a_graph(pdeip):
    """pdeip_tv_inpaint4_dev captured on a side stream after an eager call has created the workspace; replayed on changed input with
    the outputs filled beforehand, it equals the eager call bit for bit.  Red-black point SOR, the solver the drivers' graph
    replay already runs."""
    import torch

    dev = sub("device")
    truth, sparse, guide, band = ic.scene()
    kw = dict(mode=1, solver=1, outer_iter=2)
    tD, tG = up(sparse), up(guide)
    cap = dict(out=torch.zeros_like(tD), filled=torch.zeros_like(tD))

    def enqueue(o):
        dev.tv_inpaint4(tD, tG, out=o["out"], filled_out=o["filled"], **kw)

    old = pdeip.capi.get_mode()
    pdeip.capi.set_mode(1)    # the library's mode is read when the call is enqueued; keep it fixed around the capture
    try:
        enqueue(cap)   # the workspace exists before the capture
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            enqueue(cap)
        torch.cuda.current_stream().wait_stream(side)
        other = np.array(truth)
        other[20:50, 60:100] = np.nan
        other[::7, ::5] = np.nan
        for D in (other, np.array(sparse)):
            tD.copy_(up(D))
            for t in cap.values():
                t.fill_(7)   # the replay must write everything
            graph.replay()
            torch.cuda.synchronize()
            eager = dict(out=torch.zeros_like(tD), filled=torch.zeros_like(tD))
            enqueue(eager)
            torch.cuda.synchronize()
            for k in cap:
                assert cap[k].cpu().numpy().tobytes() == eager[k].cpu().numpy().tobytes(), "replay differs from the eager call in " + k
            assert np.array_equal(dev.to_matlab(cap["filled"]), np.isnan(D).astype(F32))
            assert np.isfinite(dev.to_matlab(cap["out"])).all()
    finally:
        pdeip.capi.set_mode(old)
    dev.sync_check()


def test_stereo_maps_fill(pdeip):
    """stereo_maps on the 60 x 80 pair of test_gpu_crosscheck.py: without fill the dict is what it was; with fill each view's sparse
    map comes back dense under `filled`, equal to TVinpaint4 of that map with that view's image as the guide."""
    from test_gpu_drivers import _stereo_pair

    drv = sub("drivers")
    left, right = _stereo_pair(60, 80)
    plain = drv.stereo_maps(left, right, tol=1.0)
    assert sorted(plain) == ["dense", "mask", "sparse", "stats"]
    dense = drv.DispEminND_llin_sym_2D(left, right)
    assert plain["dense"].tobytes() == dense.tobytes()
    for view in (0, 1):
        want = drv.disp_crosscheck(dense[:, :, view], dense[:, :, 1 - view], tol=1.0)
        assert np.asfortranarray(plain["sparse"][:, :, view]).tobytes() == want["sparse"].tobytes()
        assert np.asfortranarray(plain["mask"][:, :, view]).tobytes() == want["mask"].tobytes()
    fp = dict(outer_iter=3)
    maps = drv.stereo_maps(left, right, tol=1.0, fill=True, fill_param=fp)
    assert sorted(maps) == ["dense", "filled", "mask", "sparse", "stats"]
    for k in ("dense", "sparse", "mask"):
        assert maps[k].tobytes() == plain[k].tobytes(), k
    assert all(a.tobytes() == b.tobytes() for a, b in zip(maps["stats"], plain["stats"]))
    filled = maps["filled"]
    assert filled.shape == (60, 80, 2) and filled.dtype == F32 and not np.isnan(filled).any()
    known = ~np.isnan(maps["sparse"])
    assert filled[known].tobytes() == maps["sparse"][known].tobytes()
    for view, image in ((0, left), (1, right)):
        alone = drv.TVinpaint4(np.asfortranarray(maps["sparse"][:, :, view]), guide=image, **fp)
        same(filled[:, :, view], alone, "stereo_maps filled view %d" % view)
        print("stereo_maps fill, view %d: %d of 4800 pixels filled" % (view, int((~known[:, :, view]).sum())))


def test_stub_returns_the_drivers_arrays(pdeip):
    """The stub through the mock MEX runtime, as matlab/TVinpaint4_gpu.m calls it: single and double input, with and without a guide."""
    from test_flowviz_stub import call_typed
    from test_inpaint_stub import build_inpaint_stub, params

    drv = sub("drivers")
    lib = build_inpaint_stub(pdeip)
    truth, sparse, guide, band = writable_scene()
    pv = params(outer_iter=2)
    for g, gm in ((None, np.zeros((0, 0), F64)), (guide, np.array(guide))):
        want, wfilled = drv.capi_TVinpaint4(sparse, guide=g, return_filled=True, outer_iter=2)
        for D, G in ((np.array(sparse), gm), (np.array(sparse, dtype=F64), gm.astype(F64))):
            e, outs = call_typed(lib, (F32, F32), [D, G, pv])
            assert e is None
            assert outs[0].shape == sparse.shape and outs[0].tobytes(order="F") == want.tobytes(order="F")
            assert outs[1].tobytes(order="F") == wfilled.tobytes(order="F")
        e, outs = call_typed(lib, (F32,), [np.array(sparse), gm, pv])   # Dout alone
        assert e is None and outs[0].tobytes(order="F") == want.tobytes(order="F")
