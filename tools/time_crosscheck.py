"""Time disp_crosscheck and flow_crosscheck on one GPU; prints one JSON line.

    python tools/time_crosscheck.py [--reps N] [--rounds R]

The parent process never touches the GPU: it runs one child step under a time limit and stops if that fails (nothing is retried).
The child times, at 1080x1920 and 2160x3840:
  disp_crosscheck   _dev form: all outputs with statistics, all outputs without (1 launch), statistics only; host form, all outputs
  flow_crosscheck   the same four
on a smooth field (a constant displacement of 3 pixels plus noise of 0.2: a wave's gathers stay in a few columns, what a driver's
output looks like) and, for the _dev forms with statistics, on a scattered one (3 x normal: every lane gathers from another column).
Each figure is the median over R rounds of the mean of N calls (device events around the N calls of a round for the _dev forms, a
host clock around calls that return after their last copy for the host forms), after a warm-up call; the fastest and slowest round
go with it.  gbps is the bytes the call has to move per pixel (bytes_per_px: every input plane once, each output once) over that
time -- the roofline term of DESIGN 5.14; for the host forms it is the PCIe traffic instead.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
SHAPES = [(1080, 1920), (2160, 3840)]


def _child(reps, rounds):
    sys.path.insert(0, ROOT)
    import importlib

    import numpy as np
    import torch

    pkg = importlib.import_module("pde-based-image-processing_amd")
    dev = importlib.import_module("pde-based-image-processing_amd.device")
    drv = importlib.import_module("pde-based-image-processing_amd.drivers")
    capi = pkg.capi

    def dev_us(fn):
        fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(rounds):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(reps):
                fn()
            stop.record()
            torch.cuda.synchronize()
            out.append(start.elapsed_time(stop) * 1e3 / reps)
        return out

    def host_us(fn):
        fn()
        out = []
        n = max(1, reps // 10)
        for _ in range(rounds):
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            out.append((time.perf_counter() - t0) * 1e6 / n)
        return out

    def entry(us, px, bytes_per_px):
        med = statistics.median(us)
        return {"us": round(med, 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2), "bytes_per_px": bytes_per_px,
                "gbps": round(px * bytes_per_px / med / 1e3, 1)}

    def stream():
        return torch.cuda.current_stream().cuda_stream

    rng = np.random.default_rng(1)
    res = {}
    for nr, nc in SHAPES:
        px = nr * nc
        plane = lambda mean, amp: np.asfortranarray((mean + amp * rng.normal(size=(nr, nc))).astype(np.float32))
        smooth = [plane(-3.0, 0.2), plane(3.0, 0.2), plane(-1.0, 0.2), plane(1.0, 0.2)]   # forward u, v, backward u, v
        smooth = [smooth[0], smooth[2], smooth[1], smooth[3]]                            # Uf, Vf, Ub, Vb
        scattered = [plane(0.0, 3.0) for _ in range(4)]
        tS, tR = [dev.to_device(a) for a in smooth], [dev.to_device(a) for a in scattered]
        o = [torch.empty_like(tS[0]) for _ in range(3)]
        st = torch.empty(4, dtype=torch.float64, device="cuda")
        p = lambda *ts: [t.data_ptr() for t in ts]
        r = {}
        # disparity: D0 = Uf's plane, D1 = Ub's plane
        r["disp_dev_all_stats"] = entry(dev_us(lambda: dev.disp_crosscheck(tS[0], tS[2], sparse_out=o[0], mask_out=o[1], diff_out=o[2], stats_out=st)), px, 20)
        r["disp_dev_all_nostats"] = entry(dev_us(lambda: capi.call("pdeip_disp_crosscheck_dev", stream(), *p(tS[0], tS[2]), nr, nc, 1.0,
                                                                   *p(*o), None)), px, 20)
        r["disp_dev_sparse_mask_stats"] = entry(dev_us(lambda: dev.disp_crosscheck(tS[0], tS[2], sparse_out=o[0], mask_out=o[1], stats_out=st,
                                                                                   planes=False)), px, 16)
        r["disp_dev_stats_only"] = entry(dev_us(lambda: dev.disp_crosscheck(tS[0], tS[2], stats_out=st, planes=False)), px, 8)
        r["disp_dev_all_stats_scattered"] = entry(dev_us(lambda: dev.disp_crosscheck(tR[0], tR[2], sparse_out=o[0], mask_out=o[1], diff_out=o[2],
                                                                                     stats_out=st)), px, 20)
        r["disp_host_all"] = entry(host_us(lambda: drv.disp_crosscheck(smooth[0], smooth[2])), px, 20)
        r["flow_dev_all_stats"] = entry(dev_us(lambda: dev.flow_crosscheck(*tS, mask_out=o[0], err_out=o[1], stats_out=st)), px, 24)
        r["flow_dev_all_nostats"] = entry(dev_us(lambda: capi.call("pdeip_flow_crosscheck_dev", stream(), *p(*tS), nr, nc, 0.01, 0.5,
                                                                   *p(o[0], o[1]), None)), px, 24)
        r["flow_dev_stats_only"] = entry(dev_us(lambda: dev.flow_crosscheck(*tS, stats_out=st, planes=False)), px, 16)
        r["flow_dev_all_stats_scattered"] = entry(dev_us(lambda: dev.flow_crosscheck(*tR, mask_out=o[0], err_out=o[1], stats_out=st)), px, 24)
        r["flow_host_all"] = entry(host_us(lambda: drv.flow_crosscheck(*smooth)), px, 24)
        torch.cuda.synchronize()
        r["kept_smooth"] = {"disp": int(dev.disp_crosscheck(tS[0], tS[2], planes=False)[3].cpu()[0]),
                            "flow": int(dev.flow_crosscheck(*tS, planes=False)[2].cpu()[0]), "pixels": px}
        res["%dx%d" % (nr, nc)] = r
    res["device"] = torch.cuda.get_device_name(0)
    res["reps"], res["rounds"] = reps, rounds
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(_child(a.reps, a.rounds)))
        return
    step = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps),
                           "--rounds", str(a.rounds)], capture_output=True, text=True, cwd=ROOT)
    if step.returncode != 0:
        print(json.dumps({"error": "timing step exited %d: %s" % (step.returncode, step.stderr[-400:])}))
        sys.exit(1)
    print(step.stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    main()
