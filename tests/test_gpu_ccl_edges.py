"""GPU: pdeip_bwlabel_dev / pdeip_largest_component_dev on the masks of tests/ccl_edge_cases.py -- the one-workgroup form at its
limit, runs across its 64-row chunks, every pattern at a four-tile corner and astride a seam, 256..513 blocks for the scan, ties
beyond the argmax's first stride, colliding and wrapping probes of the area table -- against the flood fill of tests/ccl_ref.py,
integer for integer and bit for bit, in the forms and with the checks of test_gpu_ccl.py.  tests/test_ccl_edge_cases.py proves
that the masks reach what they claim.  Nothing here has a tolerance."""
import numpy as np
import pytest

import ccl_cases
import ccl_edge_cases as ec
from test_gpu_ccl import PAD, _dev, _run, check_case, form, reference

pytestmark = pytest.mark.gpu
R50, LATTICE_513 = "small_128x128_r50", "lattice_1026x512_513blocks"
PAST = "past_%dx%d_r50" % ec.PAST_LIMIT_SHAPE


def _params():
    out = []
    for name, A in ec.cases():
        for conn in (4, 8):
            out.append(pytest.param(name, conn, False, id="%s-conn%d-tiled" % (name, conn)))
            if ec.admits_small(A):
                out.append(pytest.param(name, conn, True, id="%s-conn%d-small" % (name, conn)))
    return out


@pytest.mark.parametrize("name,conn,small", _params())
def test_edge_cases_equal_the_flood_fill(pdeip, name, conn, small):
    check_case(pdeip, name, conn, small)


def _compare(got, name, conn, cap):
    L, num, buf, sel, num2, area, _, _ = got
    wL, wnum, wareas, wsel, warea = reference(name, conn)
    assert num == wnum and num2 == wnum and area == warea and np.array_equal(L, wL), name
    assert np.array_equal(buf[:wnum], wareas) and not buf[wnum:cap].any() and np.array_equal(buf[cap:], np.full(PAD, -7, np.int32)), name
    assert sel.tobytes() == np.ascontiguousarray(wsel).tobytes(), name


@pytest.mark.parametrize("conn", (4, 8))
def test_one_pixel_past_the_limit_runs_the_tiled_form_whatever_is_asked(pdeip, conn):
    A = ec.get(PAST)
    assert A.size == 16385
    cap = reference(PAST, conn)[1] + PAD
    with form(True):
        got = _run(pdeip, A, conn, cap)
    assert got[6] >= 5 and got[7] >= 7, "the one-workgroup form ran on a plane it does not admit (%d, %d launches)" % got[6:]
    _compare(got, PAST, conn, cap)


@pytest.mark.parametrize("small", (False, True))
@pytest.mark.parametrize("name", ("min_1x1_fg", "random_17x33_50"))
def test_areas_cap_far_beyond_one_stride_of_the_clear(pdeip, name, small):
    """5000 entries against the 256 (tiled, one block) or 1024 (small) that one stride of the clear covers: everything behind num
    comes back 0, the guard behind the cap untouched."""
    cap = 5000
    assert reference(name, 8)[1] < 256
    with form(small):
        got = _run(pdeip, ccl_cases.get(name), 8, cap)
    assert (got[6] == 1) if small else (got[6] >= 5)
    _compare(got, name, 8, cap)


@pytest.mark.parametrize("name,small", ((R50, True), ("corners_330x170", False), ("corner_arms_330x170", False)))
def test_largest_component_in_place_at_the_limit_and_on_the_corners(pdeip, name, small):
    import torch

    dev = _dev()
    lib = pdeip.capi.load()
    for conn in (4, 8):
        t = dev.to_device(np.asfortranarray(ec.get(name)))
        with form(small):
            out = dev.largest_component(t, conn, 5.0, -5.0, out=t)
        n = lib.pdeip_last_launch_count()
        torch.cuda.synchronize()
        assert (n == 1) if small else (n >= 7)
        assert out.data_ptr() == t.data_ptr()
        assert t.cpu().numpy().T.tobytes() == np.ascontiguousarray(reference(name, conn)[3]).tobytes(), (name, conn)


def test_smaller_calls_inside_the_workspace_a_larger_one_left(pdeip):
    """The workspace only grows: the 5 x 3277 plane runs inside what the 1026 x 512 one left behind, with other offsets; the small
    form in between uses none of it."""
    for name, small in ((LATTICE_513, False), (PAST, False), (R50, True), (LATTICE_513, False)):
        cap = reference(name, 8)[1] + PAD
        with form(small):
            got = _run(pdeip, ec.get(name), 8, cap)
        assert (got[6] == 1 and got[7] == 1) if small else (got[6] >= 5 and got[7] >= 7), name
        _compare(got, name, 8, cap)


def test_small_form_at_its_limit_in_a_captured_graph(pdeip):
    """bwlabel and largest_component at 128 x 128 (all of the dynamic LDS the form may ask for) captured once and replayed on
    other masks of that size, every output overwritten before each replay.  The eager call before the capture sets the
    kernel's LDS attribute, which is no stream operation."""
    import torch

    dev = _dev()
    names = (R50, "small_128x128_checker", "small_128x128_alt", R50)
    cap = max(reference(n, 8)[1] for n in names)
    with form(True):
        tA = dev.to_device(np.asfortranarray(ec.get(names[0])))
        L = torch.empty(tA.shape, dtype=torch.int32, device="cuda")
        num = torch.empty(1, dtype=torch.int32, device="cuda")
        areas = torch.empty(cap, dtype=torch.int32, device="cuda")
        sel = torch.empty_like(tA)
        num2 = torch.empty(1, dtype=torch.int32, device="cuda")
        area = torch.empty(1, dtype=torch.int32, device="cuda")

        def calls():
            dev.bwlabel(tA, 8, L, num, areas)
            dev.largest_component(tA, 8, 5.0, -5.0, out=sel, num_out=num2, area_out=area)

        calls()
        assert pdeip.capi.load().pdeip_last_launch_count() == 1
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            calls()
        torch.cuda.current_stream().wait_stream(side)
        for name in names:
            tA.copy_(dev.to_device(np.asfortranarray(ec.get(name))))
            for t in (L, num, areas, sel, num2, area):
                t.fill_(-7)  # what the replay does not write cannot pass
            graph.replay()
            torch.cuda.synchronize()
            wL, wnum, wareas, wsel, warea = reference(name, 8)
            assert int(num.item()) == wnum and int(num2.item()) == wnum and int(area.item()) == warea, name
            assert np.array_equal(L.cpu().numpy().T, wL), name
            got = areas.cpu().numpy()
            assert np.array_equal(got[:wnum], wareas) and not got[wnum:].any()
            assert sel.cpu().numpy().T.tobytes() == np.ascontiguousarray(wsel).tobytes(), name
