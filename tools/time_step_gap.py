"""The headline step (bench.py's planes, red-black iter = 4, out of place, ping-pong) with the library's profile off and on, in one
process, alternating: us per step of wall time for each, their difference (what timing the launches costs a step), and the
launch time the profile reports.  A/B two builds: PDEIP_LIB=<other libpdeip.so> python tools/time_step_gap.py [rounds [steps]]"""
import importlib, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
dev = importlib.import_module("pde-based-image-processing_amd.device")
capi = importlib.import_module("pde-based-image-processing_amd.capi")
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
U, V, coef = bench.make_planes(torch, torch.device("cuda"), bench.NROWS, bench.NCOLS)
sets = [(U, V), (torch.empty_like(U), torch.empty_like(V))]
def run(n):
    for k in range(n):
        a, b = sets[k & 1], sets[1 - (k & 1)]
        dev.oflow_sor_elin4(a[0], a[1], *coef, bench.ITER, bench.OMEGA, capi.MODE_RED_BLACK, out=b)
run(600)  # steady clocks
torch.cuda.synchronize()
wall, launch = {False: [], True: []}, []
for _ in range(rounds):
    for on in (False, True):
        capi.profile_enable(on)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(steps)
        torch.cuda.synchronize()
        wall[on].append((time.perf_counter() - t0) / steps * 1e6)
        ms, nl = capi.profile_read()
        if on:
            launch.append(ms * 1e3 / nl)
capi.profile_enable(False)
med = lambda v: sorted(v)[len(v) // 2]
print("us per step: profile off %.2f (min %.2f)   on %.2f (min %.2f)   on - off %.2f (median of pairs %.2f)   launch_us %.2f" % (
    med(wall[False]), min(wall[False]), med(wall[True]), min(wall[True]), med(wall[True]) - med(wall[False]),
    med([b - a for a, b in zip(wall[False], wall[True])]), med(launch)), flush=True)
dev.sync_check()
