"""Time the Chan-Vese AOS step (CV_solver_2d) on one GPU; prints one JSON line.

    python tools/time_cv.py [--reps N]

The parent process never touches the GPU.  It runs two child steps, each under its own time limit, and stops at the first
that fails (nothing is retried):
  1. timing: us per cv_solver call on device pointers, eager and graph-replayed, at 2160x3840x1 and at the segmentation
     drivers' scales for 15 segments, 288x384x15 (full) and 115x154x15 (rc_scl = 0.4); us per cv_terms call at the same
     shapes; and, for comparison, us per AC_solver_2d step at 2160x3840 (two sequential passes plus a re-initialisation step);
  2. `rocprofv3 --kernel-trace --stats` of the 4K calls: k_cv_lines (column and row lanes in one launch), k_cv_combine,
     k_cv_terms, next to the AC step's k_aos_col and k_aos_row, which run the same kind of chains one pass after the other.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
SHAPES = [(2160, 3840, 1), (288, 384, 15), (115, 154, 15)]
KERNELS = ("k_cv_lines", "k_cv_combine", "k_cv_terms", "k_aos_col", "k_aos_row", "k_reinit_step")


def _child_timing(reps, kernels_only):
    sys.path.insert(0, ROOT)
    import importlib

    import numpy as np
    import torch

    dev = importlib.import_module("pde-based-image-processing_amd.device")

    def timed(fn, n):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        torch.cuda.synchronize()
        start.record()
        for _ in range(n):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) * 1e3 / n  # us

    def graphed(fn, n):
        fn()
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        return timed(g.replay, n)

    rng = np.random.default_rng(1)
    res = {}
    for nr, nc, nf in (SHAPES[:1] if kernels_only else SHAPES):
        shape = (nr, nc, nf) if nf > 1 else (nr, nc)
        phi = np.asfortranarray(rng.uniform(-5, 5, shape).astype(np.float32))
        D = np.asfortranarray(rng.uniform(-1, 1, shape).astype(np.float32))
        P, Dd = dev.to_device(phi), dev.to_device(D)
        H, G, out = torch.empty_like(P), torch.empty_like(P), torch.empty_like(P)
        dev.cv_terms(P, 1.0, 1.0, 0.06, H, G)
        key = "%dx%dx%d" % (nr, nc, nf)
        r = {"cv_solver_us": timed(lambda: dev.cv_solver(P, Dd, H, G, 0.5, 0.3, out), reps),
             "cv_terms_us": timed(lambda: dev.cv_terms(P, 1.0, 1.0, 0.06, H, G), reps)}
        if not kernels_only:
            r["cv_solver_graph_us"] = graphed(lambda: dev.cv_solver(P, Dd, H, G, 0.5, 0.3, out), reps)
            r["cv_terms_graph_us"] = graphed(lambda: dev.cv_terms(P, 1.0, 1.0, 0.06, H, G), reps)
        if nf == 1:
            Df = torch.rand_like(P) + 0.1
            r["ac_solver_us"] = timed(lambda: dev.ac_solver(P, Dd, G, Df, 0.25, 1.0, out), reps)
        res[key] = r
    return res


def _kernel_split(outdir):
    """Per-kernel average durations (us) from rocprofv3's kernel stats CSV."""
    split = {}
    for path in glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row.get("Name", "")
                for key in KERNELS:
                    if key in name:
                        split[key + "_us"] = float(row["AverageNs"]) / 1e3
    return split


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--child", choices=["full", "kernels"])
    a = ap.parse_args()
    if a.child:
        print(json.dumps(_child_timing(a.reps, a.child == "kernels")))
        return
    res = {}
    me = os.path.abspath(__file__)
    step = subprocess.run(["timeout", "-k", "10", "600", sys.executable, me, "--child", "full", "--reps", str(a.reps)],
                          capture_output=True, text=True, cwd=ROOT)
    if step.returncode != 0:
        res["error"] = "timing step exited %d: %s" % (step.returncode, step.stderr[-400:])
        print(json.dumps(res))
        sys.exit(1)
    res.update(json.loads(step.stdout.strip().splitlines()[-1]))
    with tempfile.TemporaryDirectory() as tmp:
        step = subprocess.run(["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp,
                               "-o", "cv", "--", sys.executable, me, "--child", "kernels", "--reps", "5"],
                              capture_output=True, text=True, cwd=ROOT)
        if step.returncode != 0:
            res["rocprof_error"] = "rocprofv3 step exited %d: %s" % (step.returncode, step.stderr[-400:])
        else:
            split = _kernel_split(tmp)
            if "k_aos_col_us" in split and "k_aos_row_us" in split:
                split["aos_col_plus_row_us"] = split["k_aos_col_us"] + split["k_aos_row_us"]
            res["kernel_split_2160x3840"] = split
    print(json.dumps(res))
    if "rocprof_error" in res:
        sys.exit(1)


if __name__ == "__main__":
    main()
