"""Red-black iter = 4 solver calls (k_sor_rbp, out of place, ping-pong): us per call for every 5-point model at a few sizes.
A/B two builds in two processes: PDEIP_LIB=<other libpdeip.so> python tools/time_rbp.py [ROWSxCOLS ...]

    python tools/time_rbp.py --variants [ROUNDS [STEPS]] LIB[@serp] ...
times the headline step (bench.py's planes and call, as tools/time_step_gap.py does, profile off) for several builds of the
library loaded into ONE process: ROUNDS (15) rounds of one block of STEPS (200) steps per build, the builds taking turns, and per
build the median / min / max block in us per step.  LIB is a libpdeip*.so (tools/build_variant.py) or `default` for the built
library; `@serp` runs that entry with PDEIP_RBP_SERPENTINE=1.  Every entry has its own iterate planes: the timing experiments
among the variants write garbage."""
import ctypes, importlib, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
dev = importlib.import_module("pde-based-image-processing_amd.device")
capi = importlib.import_module("pde-based-image-processing_amd.capi")


def time_variants(argv):
    import bench
    nums = []
    while argv and argv[0].isdigit(): nums.append(int(argv.pop(0)))
    rounds, steps = (nums + [15, 200][len(nums):])[:2]
    U, V, coef = bench.make_planes(torch, torch.device("cuda"), bench.NROWS, bench.NCOLS)
    name = "pdeip_oflow_sor_elin4_dev_to"
    entries, libs = [], []
    for spec in argv:
        path, _, opt = spec.partition("@")
        lib = capi.load() if path == "default" else ctypes.CDLL(os.path.abspath(path))  # every library has its own state
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = capi.SIGNATURES[name], ctypes.c_int
        lib.pdeip_profile_enable.argtypes, lib.pdeip_profile_enable.restype = capi.SIGNATURES["pdeip_profile_enable"], ctypes.c_int
        lib.pdeip_profile_enable(0)
        libs.append(lib)
        entries.append((spec, fn, "1" if opt == "serp" else "0", [(U.clone(), V.clone()), (torch.empty_like(U), torch.empty_like(V))], []))
    stream, cp = dev._stream(), dev._p(*coef)
    def run(fn, sets, n):
        for k in range(n):
            a, b = sets[k & 1], sets[1 - (k & 1)]
            rc = fn(stream, *dev._p(a[0], a[1], b[0], b[1]), *cp, bench.NROWS, bench.NCOLS, bench.ITER, float(bench.OMEGA), capi.MODE_RED_BLACK, 0)
            if rc != capi.PDEIP_OK: raise capi.PdeipError(rc, "%s failed" % name)
    for r in range(rounds + 2):  # two untimed rounds: steady clocks, every kernel loaded
        for spec, fn, serp, sets, us in entries:
            os.environ["PDEIP_RBP_SERPENTINE"] = serp
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(fn, sets, steps)
            torch.cuda.synchronize()
            if r >= 2: us.append((time.perf_counter() - t0) / steps * 1e6)
    for spec, fn, serp, sets, us in entries:
        v = sorted(us)
        print("%-44s median %7.2f   min %7.2f   max %7.2f us per step (%d blocks of %d)" % (spec, v[len(v) // 2], v[0], v[-1], len(v), steps), flush=True)
    torch.cuda.synchronize()
    for lib in libs:
        if lib.pdeip_persist_error() != capi.PDEIP_OK: raise capi.PdeipError(capi.PDEIP_ERR_DEVICE, "a bounded wait timed out")


if len(sys.argv) > 1 and sys.argv[1] == "--variants":
    time_variants(sys.argv[2:])
    sys.exit(0)
sizes = [(2160, 3840), (1080, 1920), (1988, 2880)] if len(sys.argv) < 2 else [tuple(int(x) for x in a.split("x")) for a in sys.argv[1:]]
RB = capi.MODE_RED_BLACK
for nr, nc in sizes:
    g = torch.Generator(device="cuda").manual_seed(1)
    P = lambda lo, hi: torch.empty((nc, nr), device="cuda").uniform_(lo, hi, generator=g)
    a, b = [P(-1, 1), P(-1, 1)], [P(-1, 1), P(-1, 1)]
    dU, dV = P(-0.1, 0.1), P(-0.1, 0.1)
    coef = [P(-0.25, 0.25) for _ in range(3)] + [P(0.0, 0.25), P(0.0, 0.25)] + [P(0.5, 5) for _ in range(4)]
    dia = coef[3] + sum(coef[5:]) + 1
    def elin4():
        dev.oflow_sor_elin4(a[0], a[1], *coef, 4, 1.0, RB, out=(b[0], b[1]))
    def llin4():
        dev.oflow_sor_llin4(a[0], a[1], dU, dV, *coef, 4, 1.0, RB)
    def disp4():
        dev.disp_sor_llin4(a[0], dU, coef[1], coef[3], *coef[5:], 4, 1.0, RB)
    def pde4():
        dev.pde_sor4(a[0], dia, coef[1], *coef[5:], 4, 1.0, RB)
    row = []
    for fn in (elin4, llin4, disp4, pde4):
        for _ in range(200): fn()
        torch.cuda.synchronize()
        best = 1e9
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(100):
                fn()
                if fn is elin4: a, b = b, a
            torch.cuda.synchronize()
            best = min(best, (time.perf_counter() - t0) / 100)
        row.append("%s %7.1f us" % (fn.__name__, best * 1e6))
    print("%9s  %s" % ("%dx%d" % (nr, nc), "   ".join(row)), flush=True)
dev.sync_check()
