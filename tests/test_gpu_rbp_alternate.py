"""GPU: PDEIP_RBP_SERPENTINE=3 (the default on frames larger than the Infinity Cache when the variable is absent) -- every other k_sor_rbp launch on a device marches every
strip east -> west, across the launches of a call AND across calls, so that a launch starts where the one before ended
(csrc/pdeip_sor_plan.hpp, resolve_mirror).  Only the traversal order changes: every result here is compared bit for bit with the
oracle's colour order, and pdeip_debug_last_directions() shows that the launches really alternated (0: forwards, 2: mirrored).

The device's direction bit says where its last pipeline launch ended, whatever knob that launch ran under; a launch forced
forwards (knob 0) or mirrored (knob 2) therefore PINS the direction the next launch under mode 3 takes -- `pin()` below -- and
the tests that need a known first direction start from there.  PDEIP_RB_SMALL=0 throughout: small frames through the pipeline."""
import importlib

import pytest

import problems as pb
from test_gpu_seams import ENTRY, OMEGA, PLANES, knobs, want_of

pytestmark = pytest.mark.gpu


def names_of(model):
    its, ros, cfs = PLANES[model]
    return its, ros, cfs, (ros + its + cfs if model in ("llin4", "disp4") else its + cfs)


def solve(pdeip, model, d, it, col0=0, outs=None, omega=None):
    """One red-black *_dev call on the device planes d (in place, or into `outs`); returns the directions of its launches."""
    import ctypes

    import torch

    dev, capi = importlib.import_module("pde-based-image-processing_amd.device"), pdeip.capi
    its, ros, cfs, _ = names_of(model)
    first = d[its[0]]
    nrows, ncols = int(first.shape[-1]), int(first.shape[-2])
    tail = (nrows, ncols) + ((int(first.shape[0]) if first.dim() == 3 else 1,) if model == "pde4" else ())
    ptr = lambda names: [d[k].data_ptr() for k in names]
    dev._chk(*d.values(), *(outs or []))
    args = (ptr(ros) + ptr(its) if model in ("llin4", "disp4") else ptr(its)) + [o.data_ptr() for o in (outs or [])] + ptr(cfs)
    capi.call(ENTRY[model] + ("_to" if outs else ""), torch.cuda.current_stream().cuda_stream, *args, *tail, it,
              OMEGA[model] if omega is None else omega, capi.MODE_RED_BLACK, col0)
    lib = capi.load()
    buf = (ctypes.c_int * 64)()
    n = lib.pdeip_debug_last_directions(buf, 64)
    assert n == lib.pdeip_last_launch_count() and n <= 64, "one direction per launch of the chain"
    return list(buf[:n])


def on_device(pdeip, p):
    dev = importlib.import_module("pde-based-image-processing_amd.device")
    return {k: dev.to_device(v) for k, v in p.items()}


def check(pdeip, got, want, what):
    dev = importlib.import_module("pde-based-image-processing_amd.device")
    dev.sync_check()
    for k, (g, w) in enumerate(zip(got, want)):
        g = dev.to_matlab(g)
        assert pb.bit_equal(g, w), "%s, field %d: %s" % (what, k, pb.describe_mismatch(g, w))


def alternates(dirs):
    return all(a in (0, 2) for a in dirs) and all(a + b == 2 for a, b in zip(dirs, dirs[1:]))


def pin(pdeip, next_direction):
    """A small pipeline launch forced the OTHER way, so that the next launch under mode 3 runs `next_direction`."""
    d = on_device(pdeip, pb.elin4(6090, 8, 20))
    with knobs(PDEIP_RB_SMALL=0, PDEIP_RBP_SERPENTINE=2 - next_direction):
        assert solve(pdeip, "elin4", d, 4) == [2 - next_direction]


@pytest.mark.parametrize("col0", [0, 1])
def test_three_calls_ping_pong(pdeip, oracle, col0):
    """elin4 8 x 139 in two strips, the last one column wide; three calls of iter = 4, each into the other plane set (bench.py's step)."""
    import torch

    p = pb.elin4(6000, 8, 139, nan_frac=0.02)
    d = on_device(pdeip, p)
    sets = [[d["U"], d["V"]], [torch.full_like(d["U"], 7.0), torch.full_like(d["V"], 7.0)]]
    dirs = []
    with knobs(PDEIP_RB_SMALL=0, PDEIP_RBP_TJ=138, PDEIP_RBP_SERPENTINE=3):
        for k in range(3):
            a, b = sets[k & 1], sets[1 - (k & 1)]
            dirs += solve(pdeip, "elin4", dict(d, U=a[0], V=a[1]), 4, col0, outs=b)
            check(pdeip, b, want_of(oracle, "elin4", p, 4 * (k + 1), col0), "call %d, col0=%d, directions %s" % (k, col0, dirs))
    assert len(dirs) == 3 and alternates(dirs), dirs


# (model, nrows, ncols, TJ): two strips with a last one of one column; five strips with a ragged last one of 7; llin4: the read-only
# ring, three strips with a ragged last one of 13, border tiles only
CHAINS = [("elin4", 8, 139, 138), ("elin4", 8, 139, 33), ("llin4", 244, 79, 33)]


@pytest.mark.parametrize("model,nrows,ncols,tj", CHAINS, ids=["%s-%dx%d-TJ%d" % c for c in CHAINS])
def test_chains_within_a_call(pdeip, oracle, model, nrows, ncols, tj):
    """iter = 12 in place (three launches and the copy back) and iter = 8 into a destination (two launches): the oracle's bits, the
    bits of three / two calls of iter = 4, directions that alternate within the call."""
    import torch

    p = getattr(pb, model)(6100, nrows, ncols, nan_frac=0.02)
    its = PLANES[model][0]
    with knobs(PDEIP_RB_SMALL=0, PDEIP_RBP_TJ=tj, PDEIP_RBP_SERPENTINE=3):
        for it, dst in ((12, False), (8, True)):
            what = "%s %dx%d TJ=%d iter=%d %s" % (model, nrows, ncols, tj, it, "to a destination" if dst else "in place")
            want = want_of(oracle, model, p, it, 0)
            d = on_device(pdeip, p)
            outs = [torch.full_like(d[k], 7.0) for k in its] if dst else None
            dirs = solve(pdeip, model, d, it, outs=outs)
            assert len(dirs) == it // 4 and alternates(dirs), "%s: directions %s" % (what, dirs)
            check(pdeip, outs if dst else [d[k] for k in its], want, what)
            e = on_device(pdeip, p)  # the same sweeps as calls of iter = 4, in place
            steps = [solve(pdeip, model, e, 4) for _ in range(it // 4)]
            assert all(len(s) == 1 for s in steps) and alternates([s[0] for s in steps]), "%s as calls of 4: %s" % (what, steps)
            check(pdeip, [e[k] for k in its], want, what + ", as calls of iter = 4")


def test_swapped_west_east_weights_of_a_single_field_model(pdeip, oracle):
    """disp4 enters the pipeline at 2^21 pixels: 1024 x 2048 in strips of 138 columns, iter = 8: one launch each way, the mirrored
    one with wW / wE exchanged in front of derive()."""
    p = pb.disp4(6200, 1024, 2048, nan_frac=0.005)
    d = on_device(pdeip, p)
    with knobs(PDEIP_RB_SMALL=0, PDEIP_RBP_TJ=138, PDEIP_RBP_SERPENTINE=3):
        dirs = solve(pdeip, "disp4", d, 8)
    assert len(dirs) == 2 and alternates(dirs), dirs
    check(pdeip, [d["dU"]], want_of(oracle, "disp4", p, 8, 0), "disp4 1024x2048 iter=8, directions %s" % dirs)


def test_multi_frame(pdeip, oracle):
    """pde4, three frames of 1024 x 2048, iter = 8 in place: the frames of a mirrored launch are the frames of a forward one."""
    p = pb.pde4(6300, 1024, 2048, nframes=3, nan_frac=0.005)
    d = on_device(pdeip, p)
    with knobs(PDEIP_RB_SMALL=0, PDEIP_RBP_SERPENTINE=3):
        dirs = solve(pdeip, "pde4", d, 8)
    assert len(dirs) == 2 and alternates(dirs), dirs
    check(pdeip, [d["X"]], want_of(oracle, "pde4", p, 8, 0), "pde4 1024x2048x3 iter=8, directions %s" % dirs)


def test_independence_of_history(pdeip, oracle):
    """The same call after zero and after one unrelated pipeline launch: it starts in either direction and gives the same bits."""
    p, q = pb.elin4(6400, 244, 79, nan_frac=0.02), pb.elin4(6401, 8, 30)
    runs = []
    for unrelated in (0, 1):
        pin(pdeip, 2)
        d = on_device(pdeip, p)
        with knobs(PDEIP_RB_SMALL=0, PDEIP_RBP_TJ=33, PDEIP_RBP_SERPENTINE=3):
            if unrelated:
                assert solve(pdeip, "elin4", on_device(pdeip, q), 4) == [2]
            dirs = solve(pdeip, "elin4", d, 8)
        runs.append((dirs, [d["U"], d["V"]]))
    assert runs[0][0] == [2, 0] and runs[1][0] == [0, 2], [r[0] for r in runs]
    want = want_of(oracle, "elin4", p, 8, 0)
    for dirs, got in runs:
        check(pdeip, got, want, "elin4 244x79 iter=8, directions %s" % dirs)


@pytest.mark.parametrize("first", [0, 2], ids=["forward-then-mirrored", "mirrored-then-forward"])
@pytest.mark.parametrize("model", ["elin4", "llin4"])
def test_stale_ring_slots_of_the_other_direction(pdeip, oracle, model, first):
    """A launch on NaN-filled planes of another shape in one direction, then the call in the other: the loader stops S - 1 column
    groups short of what the waves read (tests/test_gpu_rbp_march.py), so those reads see the NaN the launch in front left in the
    ring -- laid down by a march the other way round -- and must reach no stored pixel.  724 rows: border and interior tiles."""
    import torch

    for ncols, tj in [(57, 16), (49, 16), (40, 9)]:
        p = getattr(pb, model)(6500 + ncols, 724, ncols, nan_frac=0.01)
        junk = {k: torch.full((ncols + 7, 724), float("nan"), device="cuda") for k in names_of(model)[3]}
        d = on_device(pdeip, p)
        pin(pdeip, first)
        with knobs(PDEIP_RB_SMALL=0, PDEIP_RBP_TJ=tj, PDEIP_RBP_SERPENTINE=3):
            assert solve(pdeip, model, junk, 4) == [first]
            dirs = solve(pdeip, model, d, 8)
        assert dirs == [2 - first, first], dirs
        check(pdeip, [d[k] for k in PLANES[model][0]], want_of(oracle, model, p, 8, 0), "%s 724x%d TJ=%d directions %s" % (model, ncols, tj, dirs))


def test_graph_replay(pdeip, oracle):
    """A captured iter = 8 call (two launches, their directions frozen into the graph) replayed twice: the bits of the eager call."""
    import torch

    dev = importlib.import_module("pde-based-image-processing_amd.device")
    graphs = importlib.import_module("pde-based-image-processing_amd.graphs")
    p = pb.elin4(6600, 8, 139, nan_frac=0.02)
    d = on_device(pdeip, p)
    coef = [d[k] for k in PLANES["elin4"][2]]

    def step(U, V):
        out = (torch.empty_like(U), torch.empty_like(V))
        dev.oflow_sor_elin4(U, V, *coef, 8, OMEGA["elin4"], pdeip.capi.MODE_RED_BLACK, out=out)
        return out

    want = want_of(oracle, "elin4", p, 8, 0)
    with knobs(PDEIP_RB_SMALL=0, PDEIP_RBP_TJ=138, PDEIP_RBP_SERPENTINE=3):
        eager = step(d["U"], d["V"])
        check(pdeip, eager, want, "eager")
        run = graphs.GraphedRun(step)
        for k in range(2):
            got = run(d["U"], d["V"])
            assert not run.failed
            check(pdeip, got, want, "replay %d" % k)
            assert all(torch.equal(a, b) for a, b in zip(got, eager))


@pytest.mark.parametrize("knob", [0, 1, 2, 3], ids=["0", "1", "2", "3"])
def test_forced_knobs_are_obeyed_on_every_launch(pdeip, oracle, knob):
    """PDEIP_RBP_SERPENTINE = 0, 1, 2: every launch runs the forced mode, whatever the device's bit says; 3 follows the bit."""
    p = pb.elin4(6700, 8, 139, nan_frac=0.02)
    want = want_of(oracle, "elin4", p, 12, 0)
    for start in (0, 2):
        pin(pdeip, start)
        d = on_device(pdeip, p)
        with knobs(PDEIP_RB_SMALL=0, PDEIP_RBP_TJ=33, PDEIP_RBP_SERPENTINE=knob):
            dirs = solve(pdeip, "elin4", d, 12)
        assert dirs == ([knob] * 3 if knob != 3 else [start, 2 - start, start]), "knob %s after a pin to %d: %s" % (knob, start, dirs)
        check(pdeip, [d["U"], d["V"]], want, "knob %s, directions %s" % (knob, dirs))


@pytest.mark.parametrize("ncols,alternate", [(2388, False), (2400, True)], ids=["below-256MiB", "above-256MiB"])
def test_default_follows_the_frame(pdeip, ncols, alternate):
    """PDEIP_RBP_SERPENTINE absent: the launches alternate where 13 planes of the frame exceed the 256 MiB of the Infinity Cache
    (2160 x 2400: 257.1 MiB; 2160 x 2388: 255.8 MiB) and all march forwards below; the bits are those of the forced forward march."""
    import torch

    dev = importlib.import_module("pde-based-image-processing_amd.device")
    g = torch.Generator(device="cuda").manual_seed(6800)
    u = lambda lo, hi: torch.empty((ncols, 2160), device="cuda").uniform_(lo, hi, generator=g)
    a, b, c = u(-0.5, 0.5), u(-0.5, 0.5), u(-1, 1)
    d = dict(U=u(-1, 1), V=u(-1, 1), M=a * b, Cu=-a * c, Cv=-b * c, Du=a * a, Dv=b * b, wW=u(0.5, 5), wN=u(0.5, 5), wE=u(0.5, 5), wS=u(0.5, 5))
    del a, b, c
    ref = dict(d, U=d["U"].clone(), V=d["V"].clone())
    pin(pdeip, 2)
    with knobs(PDEIP_RBP_SERPENTINE=None):
        dirs = solve(pdeip, "elin4", d, 8, omega=1.0)
    with knobs(PDEIP_RBP_SERPENTINE=0):
        assert solve(pdeip, "elin4", ref, 8, omega=1.0) == [0, 0]
    dev.sync_check()
    assert dirs == ([2, 0] if alternate else [0, 0]), dirs
    assert torch.equal(d["U"], ref["U"]) and torch.equal(d["V"], ref["V"])
