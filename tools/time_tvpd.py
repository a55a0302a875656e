"""Time primal-dual total variation (pdeip_tv_pd_dev) on one GPU: each kernel form per iteration, and the whole call; prints one JSON line.

    python tools/time_tvpd.py [--iter N] [--rounds R] [--no-context]

The parent process never touches the GPU: it runs one child step under a time limit and stops if that fails (nothing is retried).
The child times, at 288x384, 1080x1920 and 2160x3840, TV-L1 at lambda 0.8 on a noisy ramp with 10 % outliers:
  forms     a call of N iterations (default 200) from a given start -- no fill, nothing but the iteration's launches -- in every kernel
            form PDEIP_TVPD_STEPS selects (1: k_tvpd_step, 2 / 4 / 8: k_tvpd_block<T> with its tail of single steps), the forms
            ALTERNATING within each of the R rounds, in one process, on the same buffers.  us_per_iter is the stream time of the call
            (device events around it) over N: kernel time plus the gaps between dependent launches, not host time.  The median over the
            rounds goes with the fastest and the slowest round, whose distance is the spread a difference between forms has to exceed.
            gbps is the least traffic of an iteration over that time: 32 bytes per pixel for a single step (u, u_prev, px, py, f read;
            u, px, py written), (5 read + 4 written) * 4 / T for a block.
  call      the whole call as a user makes it: the library's choice of form, the nearest-fill start (3 launches), 300 iterations;
            call time, stream time of everything the call enqueues.
  context   drivers.TVdenoise4 (lagged-diffusivity TV, quadratic data term, red-black ordering, its defaults) on the same frame, host
            arrays in and out, wall time of one call after a warm-up: another model with another cost structure, a context figure and
            not a target.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
SHAPES = [(288, 384), (1080, 1920), (2160, 3840)]
FORMS = (1, 2, 4, 8)
KNOB = "PDEIP_TVPD_STEPS"


def _child(iters, rounds, context):
    sys.path.insert(0, ROOT)
    import importlib

    import numpy as np
    import torch

    dev = importlib.import_module("pde-based-image-processing_amd.device")
    drv = importlib.import_module("pde-based-image-processing_amd.drivers")

    def stream_us(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) * 1e3

    def entry(us, per, px=None, bytes_per_px=None):
        med = statistics.median(us) / per
        e = {"us": round(med, 2), "min_us": round(min(us) / per, 2), "max_us": round(max(us) / per, 2)}
        if bytes_per_px is not None:
            e.update(bytes_per_px=round(bytes_per_px, 2), gbps=round(px * bytes_per_px / med / 1e3, 1))
        return e

    def with_form(steps, fn):
        if steps is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = str(steps)
        try:
            return fn()
        finally:
            os.environ.pop(KNOB, None)

    rng = np.random.default_rng(1)
    res = {}
    for nr, nc in SHAPES:
        px = nr * nc
        jj, ii = np.meshgrid(np.arange(nc), np.arange(nr))
        noisy = 0.02 * ii + 0.01 * jj + 10.0 * (ii + jj > (nr + nc) // 2) + rng.normal(0.0, 0.3, (nr, nc))
        bad = rng.random((nr, nc)) < 0.10
        noisy[bad] = rng.uniform(0.0, 64.0, (nr, nc))[bad]
        host = np.asfortranarray(noisy.astype(np.float32))
        f = dev.to_device(host)
        u0, out = f.clone(), torch.empty_like(f)
        run = lambda steps: with_form(steps, lambda: dev.tv_pd(f, "l1", 0.8, iters, u0=u0, out=out))
        for steps in FORMS:     # warm-up: the workspace, the LDS opt-in
            run(steps)
        torch.cuda.synchronize()
        us = {steps: [] for steps in FORMS}
        for _ in range(rounds):
            for steps in FORMS:
                us[steps].append(stream_us(lambda: run(steps)))
        r = {"forms": {str(s): entry(us[s], iters, px, 32.0 if s == 1 else 36.0 / s + 32.0 * (iters % s) / iters) for s in FORMS}}
        call = lambda: with_form(None, lambda: dev.tv_pd(f, "l1", 0.8, 300, out=out))
        call()
        torch.cuda.synchronize()
        r["call_l1_300"] = entry([stream_us(call) for _ in range(rounds)], 1)
        if context:
            drv.TVdenoise4(host, mode=1)
            t0 = time.perf_counter()
            drv.TVdenoise4(host, mode=1)
            r["context_TVdenoise4_wall_us"] = round((time.perf_counter() - t0) * 1e6, 1)
        torch.cuda.synchronize()
        res["%dx%d" % (nr, nc)] = r
    res["device"] = torch.cuda.get_device_name(0)
    res["iter"], res["rounds"] = iters, rounds
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iter", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-context", action="store_true")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(_child(a.iter, a.rounds, not a.no_context)))
        return
    cmd = ["timeout", "-k", "10", "600", sys.executable, os.path.abspath(__file__), "--child", "--iter", str(a.iter), "--rounds", str(a.rounds)]
    step = subprocess.run(cmd + (["--no-context"] if a.no_context else []), capture_output=True, text=True, cwd=ROOT)
    if step.returncode != 0:
        print(json.dumps({"error": "timing step exited %d: %s" % (step.returncode, step.stderr[-400:])}))
        sys.exit(1)
    print(step.stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    main()
