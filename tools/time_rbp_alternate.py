"""Does marching every other k_sor_rbp launch east -> west (so that it starts where the last one ended, on lines the Infinity
Cache may still hold) change the launch?  The experiment of profiles/NOTES.md R6.1, on any build: PDEIP_RBP_SERPENTINE is read
per call, so the direction of every call is chosen here.

    python tools/time_rbp_alternate.py [ROUNDS [STEPS]]

Legs, interleaved in ONE process (blocks of STEPS (200) steps, ROUNDS (15) rounds, 300 untimed steps per leg first), profile off:
  F     knob 0 every call              today's launch
  B     knob 2 every call              control: the mirrored march by itself
  ALT   knob 0, 2, 0, 2, ...           the proposal
  ALT2  as ALT, with TWO coefficient sets of distinct memory used in turn: only the iterate can hit (elin4 at 4K only)
  M3    knob 3 every call              the library's own alternation (builds that have it: must read as ALT)
on bench.py's planes and ping-pong step (elin4, 2160 x 3840 and 1080 x 1920, iter = 4, out= the other plane set) and on
tools/time_rbp.py's disp4 and pde4 planes at 4K (in place).  Per leg: median / min / max us per step over the blocks; per leg
against F: the median and the range of the per-round (paired) differences.  ALT - F counts as an effect only if its paired
difference is larger than F's own block spread and than |B - F|."""
import importlib, os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
dev = importlib.import_module("pde-based-image-processing_amd.device")
capi = importlib.import_module("pde-based-image-processing_amd.capi")

KNOB = "PDEIP_RBP_SERPENTINE"
RB = capi.MODE_RED_BLACK
HAS_MODE3 = hasattr(capi.load(), "pdeip_debug_last_directions")
nums = [int(a) for a in sys.argv[1:] if a.isdigit()]
ROUNDS, STEPS = (nums + [15, 200][len(nums):])[:2]
WARM = 300


def knob_of(leg, k):
    return {"F": "0", "B": "2", "M3": "3"}.get(leg, "02"[k & 1])


def experiment(title, legs, call):
    """call(leg, k): step k of the leg's own sequence (the knob is set already).  Every leg keeps its own step counter, so its
    ping-pong and its directions go on from block to block."""
    count = {leg: 0 for leg in legs}
    us = {leg: [] for leg in legs}

    def block(leg, n):
        k0 = count[leg]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(k0, k0 + n):
            os.environ[KNOB] = knob_of(leg, k)
            call(leg, k)
        torch.cuda.synchronize()
        count[leg] = k0 + n
        return (time.perf_counter() - t0) / n * 1e6

    for leg in legs:
        block(leg, WARM)
    for r in range(ROUNDS):
        for leg in (legs if r % 2 == 0 else legs[::-1]):  # no leg always runs behind the same neighbour
            us[leg].append(block(leg, STEPS))
    print("%s  (%d rounds of %d steps per leg, us per step)" % (title, ROUNDS, STEPS))
    for leg in legs:
        v = sorted(us[leg])
        line = "  %-5s median %7.2f   min %7.2f   max %7.2f" % (leg, v[len(v) // 2], v[0], v[-1])
        if leg != "F":
            d = sorted(a - f for a, f in zip(us[leg], us["F"]))
            line += "   paired - F: median %+6.2f   [%+6.2f, %+6.2f]" % (d[len(d) // 2], d[0], d[-1])
        print(line, flush=True)
    f = sorted(us["F"])
    print("  yardstick: F spread %.2f, |B - F| %.2f" % (f[-1] - f[0], abs(sorted(us["B"])[len(f) // 2] - f[len(f) // 2])), flush=True)


def elin4(nrows, ncols, legs):
    device = torch.device("cuda")
    U, V, coef = bench.make_planes(torch, device, nrows, ncols)
    coefs = [coef, [t.clone() for t in coef]] if "ALT2" in legs else [coef]
    sets = {leg: [(U.clone(), V.clone()), (torch.empty_like(U), torch.empty_like(V))] for leg in legs}

    def call(leg, k):
        a, b = sets[leg][k & 1], sets[leg][1 - (k & 1)]
        dev.oflow_sor_elin4(a[0], a[1], *coefs[(k & 1) if leg == "ALT2" else 0], bench.ITER, bench.OMEGA, RB, out=b)

    experiment("elin4 %dx%d, iter = %d, ping-pong" % (nrows, ncols, bench.ITER), legs, call)


def single_field(nrows, ncols, legs):
    g = torch.Generator(device="cuda").manual_seed(1)  # tools/time_rbp.py's planes
    P = lambda lo, hi: torch.empty((ncols, nrows), device="cuda").uniform_(lo, hi, generator=g)
    a, dU = P(-1, 1), P(-0.1, 0.1)
    coef = [P(-0.25, 0.25) for _ in range(3)] + [P(0.0, 0.25), P(0.0, 0.25)] + [P(0.5, 5) for _ in range(4)]
    dia = coef[3] + sum(coef[5:]) + 1
    its = {leg: (a.clone(), dU.clone()) for leg in legs}
    experiment("disp4 %dx%d, iter = 4, in place" % (nrows, ncols), legs,
               lambda leg, k: dev.disp_sor_llin4(a, its[leg][1], coef[1], coef[3], *coef[5:], 4, 1.0, RB))
    experiment("pde4 %dx%d, iter = 4, in place" % (nrows, ncols), legs,
               lambda leg, k: dev.pde_sor4(its[leg][0], dia, coef[1], *coef[5:], 4, 1.0, RB))


capi.profile_enable(False)
extra = ["M3"] if HAS_MODE3 else []
old = os.environ.get(KNOB)
try:
    elin4(bench.NROWS, bench.NCOLS, ["F", "B", "ALT", "ALT2"] + extra)
    elin4(1080, 1920, ["F", "B", "ALT"] + extra)
    single_field(bench.NROWS, bench.NCOLS, ["F", "B", "ALT"] + extra)
finally:
    if old is None:
        os.environ.pop(KNOB, None)
    else:
        os.environ[KNOB] = old
dev.sync_check()
