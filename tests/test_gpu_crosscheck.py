"""GPU: pdeip_disp_crosscheck(_dev) and pdeip_flow_crosscheck(_dev) against the restatement (crosscheck_ref.py, pinned by
test_crosscheck_ref.py) on the seeded cases of crosscheck_cases.py.

Every case runs on planes carved at a 4-byte offset as well as on 16-byte aligned ones.

  mask, sparse, diff / err   bit for bit (NaN positions, and the bits of every other value): correctly rounded IEEE operations on
                             identical inputs in one order, plus one rounding to float32
  kept, defined, largest     bit for bit (integers in doubles; a maximum is exact in any order)
  mean                       within 2 defined 2^-53 relative of math.fsum: two summation orders of non-negative terms; and equal in
                             its bits to the sum in the documented order (reduce_tree_ref.py, pinned by test_reduce_tree_ref.py)
  launches                   2 with stats_out, 1 without
  the inputs                 unchanged; sparse_out aliasing D0 gives the same bits; two calls give identical statistics; the host forms
                             equal the _dev forms byte for byte

Measured on one MI355X (printed by the tests below, recorded in DESIGN 5.14): see the docstrings of test_stereo_maps and
test_yosemite_forward_backward.
"""
import importlib
import math

import numpy as np
import pytest

import crosscheck_cases as cc
import crosscheck_ref as cr
from flow_gpu_util import carve, check_stats, same_f32

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64


def _dev():
    return importlib.import_module("pde-based-image-processing_amd.device")


def _drv():
    return importlib.import_module("pde-based-image-processing_amd.drivers")


def _launches(pdeip):
    return pdeip.capi.load().pdeip_last_launch_count()


def _raw_stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def run_disp(pdeip, D0, D1, tol, offset):
    """The _dev form: all outputs, a second call into filled outputs, the call without statistics, sparse_out aliasing D0."""
    import torch

    dev, capi = _dev(), pdeip.capi
    t0, t1 = carve(D0, offset), carve(D1, offset)
    sparse, mask, diff, stats = dev.disp_crosscheck(t0, t1, tol=tol)
    assert _launches(pdeip) == 2
    again = dev.disp_crosscheck(t0, t1, tol=tol, sparse_out=torch.full_like(t0, 5.0), mask_out=torch.full_like(t0, 5.0),
                                diff_out=torch.full_like(t0, 5.0), stats_out=torch.full((4,), 5.0, dtype=torch.float64, device="cuda"))
    alone = torch.full_like(t0, 5.0)
    rows, cols = D0.shape
    capi.call("pdeip_disp_crosscheck_dev", _raw_stream(), t0.data_ptr(), t1.data_ptr(), rows, cols, float(tol), None, alone.data_ptr(), None, None)
    assert _launches(pdeip) == 1
    inplace = carve(D0, offset)
    dev.disp_crosscheck(inplace, t1, tol=tol, sparse_out=inplace, planes=False)
    torch.cuda.synchronize()
    assert capi.last_error() == ""
    assert dev.to_matlab(t0).tobytes() == D0.tobytes() and dev.to_matlab(t1).tobytes() == D1.tobytes(), "an input was modified"
    out = [dev.to_matlab(sparse), dev.to_matlab(mask), dev.to_matlab(diff), stats.cpu().numpy()]
    for k in range(3):
        assert dev.to_matlab(again[k]).tobytes() == out[k].tobytes(), "two calls differ in output %d" % k
    assert again[3].cpu().numpy().tobytes() == out[3].tobytes(), "two calls differ in their statistics"
    assert dev.to_matlab(alone).tobytes() == out[1].tobytes(), "the mask of the call without statistics differs"
    assert dev.to_matlab(inplace).tobytes() == out[0].tobytes(), "sparse_out aliasing D0 differs"
    return out


@pytest.mark.parametrize("kind", cc.DISP_KINDS)
@pytest.mark.parametrize("shape", cc.DISP_SHAPES, ids=cc.shape_id)
def test_disp_crosscheck_equals_the_restatement(pdeip, shape, kind):
    D0, D1, tols = cc.disp_case(shape, kind)
    for tol in tols:
        want = cr.disp_crosscheck(D0, D1, tol)
        for offset in (0, 1):
            what = "disparity %s %s tol %g offset %d" % (shape, kind, tol, offset)
            sparse, mask, diff, stats = run_disp(pdeip, D0, D1, tol, offset)
            assert np.array_equal(mask, want["mask"]), "%s: the mask differs at %d pixels" % (what, int((mask != want["mask"]).sum()))
            same_f32(sparse, want["sparse"], what + " sparse")
            same_f32(diff, want["diff"], what + " diff")
            check_stats(stats, want, what)
    if kind == "constant":
        assert stats[0] == stats[1] == shape[0] * (shape[1] - 1) and stats[2] == 0.0 and stats[3] == 0.0
    if kind == "neg_zero":
        at = cc.lace_positions(shape)
        flat = sparse.reshape(-1, order="F")
        assert all(np.signbit(flat[p]) for p in at if not np.isnan(flat[p])) and any(not np.isnan(flat[p]) for p in at)


def run_flow(pdeip, planes, a, b, offset):
    import torch

    dev, capi = _dev(), pdeip.capi
    ts = [carve(p, offset) for p in planes]
    mask, err, stats = dev.flow_crosscheck(*ts, a=a, b=b)
    assert _launches(pdeip) == 2
    again = dev.flow_crosscheck(*ts, a=a, b=b, mask_out=torch.full_like(ts[0], 5.0), err_out=torch.full_like(ts[0], 5.0),
                                stats_out=torch.full((4,), 5.0, dtype=torch.float64, device="cuda"))
    alone = torch.full_like(ts[0], 5.0)
    rows, cols = planes[0].shape
    capi.call("pdeip_flow_crosscheck_dev", _raw_stream(), *[t.data_ptr() for t in ts], rows, cols, float(a), float(b), None, alone.data_ptr(), None)
    assert _launches(pdeip) == 1
    torch.cuda.synchronize()
    assert capi.last_error() == ""
    for t, p in zip(ts, planes):
        assert dev.to_matlab(t).tobytes() == p.tobytes(), "an input was modified"
    out = [dev.to_matlab(mask), dev.to_matlab(err), stats.cpu().numpy()]
    for k in range(2):
        assert dev.to_matlab(again[k]).tobytes() == out[k].tobytes(), "two calls differ in output %d" % k
    assert again[2].cpu().numpy().tobytes() == out[2].tobytes(), "two calls differ in their statistics"
    assert dev.to_matlab(alone).tobytes() == out[1].tobytes(), "the error plane of the call without statistics differs"
    return out


@pytest.mark.parametrize("kind", cc.FLOW_KINDS)
@pytest.mark.parametrize("shape", cc.FLOW_SHAPES, ids=cc.shape_id)
def test_flow_crosscheck_equals_the_restatement(pdeip, shape, kind):
    *planes, params = cc.flow_case(shape, kind)
    for a, b in params:
        want = cr.flow_crosscheck(*planes, a, b)
        for offset in (0, 1):
            what = "flow %s %s a %g b %g offset %d" % (shape, kind, a, b, offset)
            mask, err, stats = run_flow(pdeip, planes, a, b, offset)
            assert np.array_equal(mask, want["mask"]), "%s: the mask differs at %d pixels" % (what, int((mask != want["mask"]).sum()))
            same_f32(err, want["err"], what + " err")
            check_stats(stats, want, what)
    if kind == "constant":
        assert stats[0] == stats[1] == (shape[0] - 1) * (shape[1] - 1) and stats[2] == 0.0 and stats[3] == 0.0


def test_host_forms_equal_the_dev_forms(pdeip):
    drv = _drv()
    for shape in ((37, 53), (257, 3)):
        for kind in ("normal", "nonfinite_gathered", "edges"):
            D0, D1, tols = cc.disp_case(shape, kind)
            got = drv.disp_crosscheck(D0, D1, tol=tols[0])
            assert pdeip.capi.last_error() == ""
            sparse, mask, diff, stats = run_disp(pdeip, D0, D1, tols[0], 0)
            assert got["sparse"].tobytes() == sparse.tobytes() and got["mask"].tobytes() == mask.tobytes() and got["diff"].tobytes() == diff.tobytes()
            assert np.array([got["kept"], got["defined"], got["mean"], got["max"]], F64).tobytes() == stats.tobytes()
            *planes, params = cc.flow_case(shape, kind)
            got = drv.flow_crosscheck(*planes, a=params[0][0], b=params[0][1])
            assert pdeip.capi.last_error() == ""
            mask, err, stats = run_flow(pdeip, planes, params[0][0], params[0][1], 0)
            assert got["mask"].tobytes() == mask.tobytes() and got["err"].tobytes() == err.tobytes()
            assert np.array([got["kept"], got["defined"], got["mean"], got["max"]], F64).tobytes() == stats.tobytes()
    # the wrappers' defaults are the header's: tol 1, a 0.01, b 0.5
    D0, D1, _ = cc.disp_case((37, 53), "normal")
    assert drv.disp_crosscheck(D0, D1)["kept"] == cr.disp_crosscheck(D0, D1, 1.0)["kept"]
    *planes, _ = cc.flow_case((37, 53), "normal")
    assert drv.flow_crosscheck(*planes)["kept"] == cr.flow_crosscheck(*planes, 0.01, 0.5)["kept"]


def test_captured_in_a_graph(pdeip):
    """Both _dev calls in one captured graph on a side stream, after an eager call has created the workspace; replayed on changed
    inputs with every output filled beforehand, it equals the eager calls bit for bit."""
    import torch

    dev = _dev()
    shape = (270, 480)
    kinds = ["normal", "nonfinite_gathered", "edges"]
    tD = [dev.to_device(p) for p in cc.disp_case(shape, kinds[0])[:2]]
    tF = [dev.to_device(p) for p in cc.flow_case(shape, kinds[0])[:4]]

    def fresh():
        plane = lambda: torch.zeros_like(tD[0])
        stats = lambda: torch.zeros(4, dtype=torch.float64, device="cuda")
        return dict(sparse=plane(), dmask=plane(), diff=plane(), dstats=stats(), fmask=plane(), err=plane(), fstats=stats())

    def enqueue(o):
        dev.disp_crosscheck(*tD, tol=2.0, sparse_out=o["sparse"], mask_out=o["dmask"], diff_out=o["diff"], stats_out=o["dstats"])
        dev.flow_crosscheck(*tF, a=0.5, b=2.0, mask_out=o["fmask"], err_out=o["err"], stats_out=o["fstats"])

    cap = fresh()
    enqueue(cap)   # the workspace exists before the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        enqueue(cap)
    torch.cuda.current_stream().wait_stream(side)
    for kind in kinds[1:]:
        for t, p in zip(tD, cc.disp_case(shape, kind)[:2]):
            t.copy_(dev.to_device(p))
        for t, p in zip(tF, cc.flow_case(shape, kind)[:4]):
            t.copy_(dev.to_device(p))
        for t in cap.values():
            t.fill_(7)   # the replay must write everything
        graph.replay()
        torch.cuda.synchronize()
        eager = fresh()
        enqueue(eager)
        torch.cuda.synchronize()
        for k in cap:
            assert cap[k].cpu().numpy().tobytes() == eager[k].cpu().numpy().tobytes(), "replay differs from the eager call in " + k
        want = cr.disp_crosscheck(*cc.disp_case(shape, kind)[:2], 2.0)
        assert cap["dstats"].cpu().numpy()[0] == want["kept"] and np.array_equal(dev.to_matlab(cap["dmask"]), want["mask"])


def test_stereo_maps(pdeip):
    """drivers.stereo_maps on a textured 60 x 80 pair whose second view is the first shifted by 3 columns.  The kept share is printed,
    not asserted: nobody has measured what it should be.  On one MI355X: see DESIGN 5.14."""
    from test_gpu_drivers import _stereo_pair

    drv = _drv()
    left, right = _stereo_pair(60, 80)
    maps = drv.stereo_maps(left, right, tol=1.0)
    dense = drv.DispEminND_llin_sym_2D(left, right)
    assert maps["dense"].shape == (60, 80, 2) and maps["dense"].tobytes() == dense.tobytes()
    for view in (0, 1):
        want = drv.disp_crosscheck(dense[:, :, view], dense[:, :, 1 - view], tol=1.0)
        assert np.asfortranarray(maps["sparse"][:, :, view]).tobytes() == want["sparse"].tobytes()
        assert np.asfortranarray(maps["mask"][:, :, view]).tobytes() == want["mask"].tobytes()
        assert maps["stats"][view].tobytes() == np.array([want["kept"], want["defined"], want["mean"], want["max"]], F64).tobytes()
        print("stereo_maps 60x80, shift 3, tol 1: view %d keeps %d of %d pixels (%.3f), %d defined, mean |r| %.4f, largest %.4f"
              % (view, want["kept"], 4800, want["kept"] / 4800.0, want["defined"], want["mean"], want["max"]))
    sp = np.asfortranarray(maps["sparse"][:, :, 0])
    med = drv.nanmedfilt2(sp)
    assert med.shape == sp.shape and med.dtype == F32
    pyr = drv.sparse_pyramid(sp)
    assert len(pyr) >= 1 and pyr[0].tobytes() == med.tobytes()
    other = drv.stereo_maps(left, right, tol=0.25, firstLoop=2)   # parameters reach the driver, tol the check
    assert other["dense"].tobytes() == drv.DispEminND_llin_sym_2D(left, right, firstLoop=2).tobytes()


def test_yosemite_forward_backward(pdeip, oracle):
    """The late-linearisation flow of tests/test_yosemite.py, forward and with the frames swapped, left on the device and cross-checked
    there with the defaults (a = 0.01, b = 0.5); the mask then restricts device.flow_errors.  The masked and unmasked mean endpoint
    errors are printed, and no inequality between them is asserted.  On one MI355X: see DESIGN 5.14."""
    import torch

    import test_yosemite as ty

    dev = _dev()
    fl = importlib.import_module("pde-based-image-processing_amd.flow_level")
    py = importlib.import_module("pde-based-image-processing_amd.pyramid")
    I0, I1, Ut, Vt = ty._data()
    level = fl.FlowLlinLevel(ty.PARAM, mode=pdeip.MODE_EXACT_ORDER)

    def resident_flow(A, B):
        P0, P1 = py.build(A, B)
        last = {}

        def run_level(a, b, U, V):
            gU, gV = level.run(dev.to_device(a), dev.to_device(b), dev.to_device(U), dev.to_device(V))
            last["U"], last["V"] = gU, gV
            return dev.to_matlab(gU), dev.to_matlab(gV)

        py.coarse_to_fine(P0, P1, run_level)
        return last["U"].contiguous(), last["V"].contiguous()

    gUf, gVf = resident_flow(I0, I1)
    gUb, gVb = resident_flow(I1, I0)
    mask, err, stats = dev.flow_crosscheck(gUf, gVf, gUb, gVb)
    tUt, tVt = dev.to_device(Ut), dev.to_device(Vt)
    _, _, masked = dev.flow_errors(gUf, gVf, tUt, tVt, mask=mask, planes=False)
    _, _, plain = dev.flow_errors(gUf, gVf, tUt, tVt, planes=False)
    torch.cuda.synchronize()
    stats, masked, plain = stats.cpu().numpy(), masked.cpu().numpy(), plain.cpu().numpy()
    m = dev.to_matlab(mask)
    n = m.size
    assert set(np.unique(m)) <= {0.0, 1.0} and float(m.astype(F64).sum()) == stats[0]
    want = cr.flow_crosscheck(*[dev.to_matlab(t) for t in (gUf, gVf, gUb, gVb)], 0.01, 0.5)
    assert np.array_equal(m, want["mask"]) and stats[1] == want["defined"]
    check_stats(stats, want, "yosemite forward-backward")
    assert masked[0] == int(((m != 0) & np.isfinite(Ut) & np.isfinite(Vt)).sum())
    print("yosemite forward-backward, a 0.01 b 0.5: kept %d of %d pixels (%.3f), %d defined, mean |f + b| %.4f, largest %.4f; mean endpoint "
          "error %.4f over the kept pixels, %.4f over all %d"
          % (stats[0], n, stats[0] / n, stats[1], stats[2], stats[3], masked[1], plain[1], plain[0]))


def test_stubs_return_the_drivers_arrays(pdeip):
    """Both stubs through the mock MEX runtime, as the matlab/*.m wrappers call them: single and double input."""
    from test_flowviz_stub import build_flow_stub, call_typed

    drv = _drv()
    lib = build_flow_stub("disp_crosscheck_gpu", pdeip)
    D0, D1, _ = cc.disp_case((37, 53), "nonfinite_gathered")
    want = drv.disp_crosscheck(D0, D1, tol=2.0)
    wstats = np.array([want["kept"], want["defined"], want["mean"], want["max"]], F64)
    for a, b in ((D0, D1), (D0.astype(F64), D1.astype(F64)), (D0, D1.astype(F64))):
        e, outs = call_typed(lib, (F32, F32, F64), [a, b, np.array([2.0])])
        assert e is None
        assert outs[0].tobytes(order="F") == want["sparse"].tobytes(order="F") and outs[1].tobytes(order="F") == want["mask"].tobytes(order="F")
        assert outs[2].shape == (1, 4) and outs[2].tobytes() == wstats.tobytes()
    e, outs = call_typed(lib, (F32,), [D0, D1, np.array([2.0])])   # Ds alone
    assert e is None and outs[0].tobytes(order="F") == want["sparse"].tobytes(order="F")

    lib = build_flow_stub("flow_crosscheck_gpu", pdeip)
    Uf, Vf, Ub, Vb, _ = cc.flow_case((37, 53), "nonfinite_gathered")
    want = drv.flow_crosscheck(Uf, Vf, Ub, Vb, a=0.5, b=2.0)
    wstats = np.array([want["kept"], want["defined"], want["mean"], want["max"]], F64)
    fwd, bwd = np.asfortranarray(np.stack([Uf, Vf], axis=2)), np.asfortranarray(np.stack([Ub, Vb], axis=2))
    for a, b in ((fwd, bwd), (fwd.astype(F64), bwd.astype(F64))):
        e, outs = call_typed(lib, (F32, F32, F64), [a, b, np.array([0.5, 2.0])])
        assert e is None
        assert outs[0].shape == (37, 53) and outs[0].tobytes(order="F") == want["mask"].tobytes(order="F")
        assert outs[1].tobytes(order="F") == want["err"].tobytes(order="F")
        assert outs[2].shape == (1, 4) and outs[2].tobytes() == wstats.tobytes()
    e, outs = call_typed(lib, (F32,), [fwd, bwd, np.array([0.5, 2.0])])   # mask alone
    assert e is None and outs[0].tobytes(order="F") == want["mask"].tobytes(order="F")
