"""Time the hole filling (csrc/pdeip_inpaint.hip) on one GPU; prints one JSON line per frame size.

    python tools/time_inpaint.py [--reps N] [--rounds R] [--shapes 288x384,1080x1920,2160x3840]

The parent process never touches the GPU: it runs one child step under a time limit and stops if that fails (nothing is retried).
The child times, on a smooth single-frame map with 15 % holes (a band of 5 % of the columns, a border strip of 2 %, 8 % random pixels)
and a one-channel guide:
  stages      nan_resize (to the next level's size), inpaint_meanfill, tv4_inpaint_assemble with and without the guide, tv4_assemble
              on the same planes (the denoiser's kernel, for comparison), inpaint_merge, and one solver call (inner_iter 5, omega 1.75)
              of the finest level: pde_alr4 and pde_sor4, red-black and exact order
  levels      per level of the default pyramid one assembly and one pde_alr4 call in red-black order, times outer_iter + 1: where the
              driver's time goes (a composition of separately timed calls, not a trace)
  driver      device.tv_inpaint4 with the defaults on resident planes, red-black and exact order; drivers.capi_TVinpaint4 through host
              pointers, red-black
Each figure is the median over R rounds of the mean of N calls (device events around the N calls of a round for resident calls, a host
clock around calls that return after their last copy for the host form), after a warm-up call; the fastest and slowest round go with
it.  gbps is bytes_per_px (every input plane read once, every output written once: the roofline term of DESIGN 5.15) over that time.
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
DEFAULT_SHAPES = "288x384,1080x1920,2160x3840"


def _child(reps, rounds, shapes):
    sys.path.insert(0, ROOT)
    import importlib

    import numpy as np
    import torch

    pkg = importlib.import_module("pde-based-image-processing_amd")
    dev = importlib.import_module("pde-based-image-processing_amd.device")
    drv = importlib.import_module("pde-based-image-processing_amd.drivers")
    RB, EXACT = pkg.MODE_RED_BLACK, pkg.MODE_EXACT_ORDER

    def dev_us(fn, n):
        fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(rounds):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(n):
                fn()
            stop.record()
            torch.cuda.synchronize()
            out.append(start.elapsed_time(stop) * 1e3 / n)
        return out

    def host_us(fn, n):
        fn()
        out = []
        for _ in range(rounds):
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            out.append((time.perf_counter() - t0) * 1e6 / n)
        return out

    def entry(us, px=None, bytes_per_px=None):
        med = statistics.median(us)
        e = {"us": round(med, 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2)}
        if px:
            e.update(bytes_per_px=bytes_per_px, gbps=round(px * bytes_per_px / med / 1e3, 1))
        return e

    def scene(nr, nc, seed):
        rng = np.random.default_rng(seed)
        jj, ii = np.meshgrid(np.arange(nc), np.arange(nr))
        truth = 20.0 + 8.0 * np.sin(ii / (0.21 * nr)) * np.cos(jj / (0.17 * nc)) + 10.0 * (jj > 0.55 * nc)
        guide = 0.35 + 0.04 * np.sin(0.31 * ii) * np.cos(0.23 * jj) + 0.4 * (jj > 0.55 * nc)
        hole = rng.random((nr, nc)) < 0.08
        hole[:, int(0.50 * nc):int(0.55 * nc)] = True
        hole[:, :max(1, int(0.02 * nc))] = True
        D = np.where(hole, np.nan, truth)
        return np.asfortranarray(D.astype(np.float32)), np.asfortranarray(guide.astype(np.float32)), float(hole.mean())

    for nr, nc in shapes:
        px = nr * nc
        n_fast = reps
        n_solve = max(2, reps // 10)
        n_driver = 1 if px > 3000000 else (2 if px > 500000 else max(2, reps // 10))
        D, guide, share = scene(nr, nc, 1)
        tD, tG = dev.to_device(D), dev.to_device(guide)
        r = {"shape": "%dx%d" % (nr, nc), "holes": round(share, 4)}
        nr1, nc1 = int(math.ceil(nr * 0.75)), int(math.ceil(nc * 0.75))
        X = dev.inpaint_meanfill(tD)
        TRACE, B = torch.empty_like(X), torch.empty_like(X)
        w4 = [torch.empty_like(X) for _ in range(4)]
        out, filled = torch.empty_like(X), torch.empty_like(X)
        st = {}
        st["nan_resize"] = entry(dev_us(lambda: dev.nan_resize(tD, nr1, nc1, 0.25), n_fast), px, 4 + 4 * 0.5625)
        st["pyr_resize"] = entry(dev_us(lambda: dev.pyr_resize(tD, nr1, nc1), n_fast), px, 4 + 4 * 0.5625)
        st["inpaint_meanfill"] = entry(dev_us(lambda: dev.inpaint_meanfill(tD, out=out), n_fast), px, 12)   # D twice (sum, then fill), out once
        st["tv4_inpaint_assemble_guide"] = entry(dev_us(lambda: dev.tv4_inpaint_assemble(X, tD, 5.0, TRACE, B, w4, tG, 20.0), n_fast), px, 36)
        st["tv4_inpaint_assemble"] = entry(dev_us(lambda: dev.tv4_inpaint_assemble(X, tD, 5.0, TRACE, B, w4), n_fast), px, 32)
        st["tv4_assemble"] = entry(dev_us(lambda: dev.tv4_assemble(X, X, 5.0, TRACE, B, w4), n_fast), px, 32)
        st["inpaint_merge"] = entry(dev_us(lambda: dev.inpaint_merge(X, tD, out=out, filled_out=filled), n_fast), px, 16)
        dev.tv4_inpaint_assemble(X, tD, 5.0, TRACE, B, w4, tG, 20.0)
        for name, fn, mode in (("pde_alr4_red_black", dev.pde_alr4, RB), ("pde_sor4_red_black", dev.pde_sor4, RB),
                               ("pde_alr4_exact", dev.pde_alr4, EXACT), ("pde_sor4_exact", dev.pde_sor4, EXACT)):
            Y = X.clone()
            st[name] = entry(dev_us(lambda: fn(Y, TRACE, B, w4[0], w4[1], w4[2], w4[3], 5, 1.75, mode), n_solve))
        r["stages"] = st
        # the default pyramid, level by level: one assembly and one red-black pde_alr4 call, times outer_iter + 1 = 11
        sizes = [(nr, nc)]
        while True:
            a, b = sizes[-1]
            a1, b1 = int(math.ceil(a * 0.75)), int(math.ceil(b * 0.75))
            if min(a1, b1) < 16:
                break
            sizes.append((a1, b1))
        lv, Dk, Gk = [], tD, tG
        for k, (a, b) in enumerate(sizes):
            if k:
                Dk, Gk = dev.nan_resize(Dk, a, b, 0.25), dev.pyr_resize(Gk, a, b)
            Xk = dev.inpaint_meanfill(Dk)
            Tk, Bk = torch.empty_like(Xk), torch.empty_like(Xk)
            wk = [torch.empty_like(Xk) for _ in range(4)]
            n = n_solve if k == 0 else max(n_solve, 10)
            asm = statistics.median(dev_us(lambda: dev.tv4_inpaint_assemble(Xk, Dk, 5.0, Tk, Bk, wk, Gk, 20.0), n))
            sol = statistics.median(dev_us(lambda: dev.pde_alr4(Xk, Tk, Bk, wk[0], wk[1], wk[2], wk[3], 5, 1.75, RB), n))
            lv.append({"size": "%dx%d" % (a, b), "assemble_us_x11": round(11 * asm, 1), "solver_us_x11": round(11 * sol, 1)})
        new_us = sum(l["assemble_us_x11"] for l in lv)
        sol_us = sum(l["solver_us_x11"] for l in lv)
        r["levels"] = lv
        r["composed_red_black"] = {"solver_us": round(sol_us, 1), "assemble_us": round(new_us, 1),
                                   "solver_share": round(sol_us / (sol_us + new_us), 3),
                                   "finest_solver_share": round(lv[0]["solver_us_x11"] / (sol_us + new_us), 3)}
        dr = {}
        dr["dev_red_black"] = entry(dev_us(lambda: dev.tv_inpaint4(tD, tG, out=out, filled_out=filled, mode=RB), n_driver))
        dr["dev_red_black_no_guide"] = entry(dev_us(lambda: dev.tv_inpaint4(tD, None, out=out, filled_out=filled, mode=RB), n_driver))
        dr["dev_exact"] = entry(dev_us(lambda: dev.tv_inpaint4(tD, tG, out=out, filled_out=filled, mode=EXACT), n_driver))
        dr["host_red_black"] = entry(host_us(lambda: drv.capi_TVinpaint4(D, guide=guide, mode=RB, return_filled=True), n_driver), px, 16)
        dev.tv_inpaint4(tD, tG, out=out, mode=RB)
        dr["launches_red_black"] = pkg.capi.load().pdeip_last_launch_count()
        dev.sync_check()
        r["driver"] = dr
        r["device"] = torch.cuda.get_device_name(0)
        r["reps"], r["rounds"] = reps, rounds
        print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default=DEFAULT_SHAPES)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        _child(a.reps, a.rounds, [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")])
        return
    # the child's lines pass through as they come, so the sizes already timed survive a later failure
    step = subprocess.run(["timeout", "-k", "10", "900", sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps),
                           "--rounds", str(a.rounds), "--shapes", a.shapes], cwd=ROOT)
    if step.returncode != 0:
        print(json.dumps({"error": "timing step exited %d" % step.returncode}))
        sys.exit(1)


if __name__ == "__main__":
    main()
