"""Time flow2color and flow_errors on one GPU; prints one JSON line.

    python tools/time_flowviz.py [--reps N] [--rounds R]

The parent process never touches the GPU: it runs one child step under a time limit and stops if that fails (nothing is retried).
The child times, at 1080x1920 and 2160x3840 on a seeded normal flow with runme.m's border of 10:
  flow2color   _dev form: float and uint8 output, automatic and given maximum; host form: float and uint8 (with its transfers)
  flow_errors  _dev form: with the two error planes and statistics only; host form with the planes
Each figure is the median over R rounds of the mean of N calls (device events around the N calls of a round for the _dev forms, a
host clock around calls that return after their last copy for the host forms), after a warm-up call; the fastest and slowest round
go with it.  gbps is the bytes the call has to move per pixel (bytes_per_px: U and V once per pass that reads them, each output
once) over that time -- the roofline term of DESIGN 5.13; for the host forms it is the PCIe traffic instead.
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
BORDER = 10


def _child(reps, rounds):
    sys.path.insert(0, ROOT)
    import importlib

    import numpy as np
    import torch

    dev = importlib.import_module("pde-based-image-processing_amd.device")
    drv = importlib.import_module("pde-based-image-processing_amd.drivers")

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

    rng = np.random.default_rng(1)
    res = {}
    for nr, nc in SHAPES:
        U, V, Ut, Vt = [np.asfortranarray((3.0 * rng.normal(size=(nr, nc))).astype(np.float32)) for _ in range(4)]
        flow = np.stack([U, V], axis=2)
        tU, tV, tUt, tVt = [dev.to_device(a) for a in (U, V, Ut, Vt)]
        br, bc = nr + 2 * BORDER, nc + 2 * BORDER
        px, bpx = nr * nc, br * bc
        f32 = torch.empty((3, bc, br), dtype=torch.float32, device="cuda")
        u8 = torch.empty((br, bc, 3), dtype=torch.uint8, device="cuda")
        mv = torch.empty(1, dtype=torch.float64, device="cuda")
        epe, ang = torch.empty_like(tU), torch.empty_like(tU)
        st = torch.empty(4, dtype=torch.float64, device="cuda")
        grow = bpx / px   # output pixels per flow pixel
        r = {}
        r["flow2color_dev_float_auto"] = entry(dev_us(lambda: dev.flow2color(tU, tV, border=BORDER, out=f32, maxvalue_out=mv)), px, 16 + 12 * grow)
        r["flow2color_dev_float_given"] = entry(dev_us(lambda: dev.flow2color(tU, tV, maxvalue=9.0, border=BORDER, out=f32, maxvalue_out=mv)), px, 8 + 12 * grow)
        r["flow2color_dev_uint8_auto"] = entry(dev_us(lambda: dev.flow2color(tU, tV, border=BORDER, uint8=True, out=u8, maxvalue_out=mv)), px, 16 + 3 * grow)
        r["flow2color_dev_uint8_given"] = entry(dev_us(lambda: dev.flow2color(tU, tV, maxvalue=9.0, border=BORDER, uint8=True, out=u8, maxvalue_out=mv)), px, 8 + 3 * grow)
        r["flow_errors_dev_planes"] = entry(dev_us(lambda: dev.flow_errors(tU, tV, tUt, tVt, epe_out=epe, ang_out=ang, stats_out=st)), px, 24)
        r["flow_errors_dev_stats_only"] = entry(dev_us(lambda: dev.flow_errors(tU, tV, tUt, tVt, stats_out=st, planes=False)), px, 16)
        r["flow2color_host_float"] = entry(host_us(lambda: drv.flow2color(flow, border=BORDER)), px, 8 + 12 * grow)
        r["flow2color_host_uint8"] = entry(host_us(lambda: drv.flow2color(flow, border=BORDER, uint8=True)), px, 8 + 3 * grow)
        r["flow_errors_host_planes"] = entry(host_us(lambda: drv.flow_errors(U, V, Ut, Vt)), px, 24)
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
