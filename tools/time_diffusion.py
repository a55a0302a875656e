"""Time Diffusion4_v10 (pdeip_diffusion4_dev) on one GPU; prints one JSON line.

    python tools/time_diffusion.py [--reps N]

The parent process never touches the GPU.  It runs two child steps, each under its own time limit, and stops at the first
that fails (nothing is retried):
  1. timing: us per diffusion4 call on device pointers with the driver's defaults (alpha 25, 6 outer iterations), eager and
     graph-replayed, at 2160x3840x1, 2160x3840x3, 1080x1920x3 and 320x400x3 (the drivsco size); and, as the yardstick of the
     line launch, us per CV_solver_2d call at 2160x3840x1 in the same process;
  2. `rocprofv3 --kernel-trace --stats` of one 4K gray call of each: k_diffweights6, k_diff4_lines and k_diff4_combine next to
     k_cv_lines, which runs chains of the same lengths with the same chain arithmetic; lines_ratio = k_diff4_lines / k_cv_lines.
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
SHAPES = [(2160, 3840, 1), (2160, 3840, 3), (1080, 1920, 3), (320, 400, 3)]
KERNELS = ("k_diffweights6", "k_diff4_lines", "k_diff4_combine", "k_cv_lines", "k_cv_combine")


def _image(rng, shape):
    import numpy as np

    blocks = rng.uniform(0, 255, (shape[0] // 16 + 1, shape[1] // 16 + 1) + tuple(shape[2:]))
    I = blocks[np.arange(shape[0]) // 16][:, np.arange(shape[1]) // 16] + rng.normal(0, 6, shape)
    return np.asfortranarray(np.clip(I, 0, 255).astype(np.float32))


def _child_timing(reps, kernels_only):
    sys.path.insert(0, ROOT)
    import importlib

    import numpy as np
    import torch

    dev = importlib.import_module("pde-based-image-processing_amd.device")
    nan = float("nan")

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
        I = dev.to_device(_image(rng, shape))
        out = torch.empty_like(I)
        key = "%dx%dx%d" % (nr, nc, nf)
        if kernels_only:
            dev.diffusion4(I, nan, nan, out)
            torch.cuda.synchronize()
            continue
        res[key] = {"diffusion4_us": timed(lambda: dev.diffusion4(I, nan, nan, out), reps),
                    "diffusion4_graph_us": graphed(lambda: dev.diffusion4(I, nan, nan, out), reps)}
    # the yardstick: one CV_solver_2d step at 4K gray (k_cv_lines + k_cv_combine)
    phi = np.asfortranarray(rng.uniform(-5, 5, (2160, 3840)).astype(np.float32))
    D = np.asfortranarray(rng.uniform(-1, 1, (2160, 3840)).astype(np.float32))
    P, Dd = dev.to_device(phi), dev.to_device(D)
    H, G, o = torch.empty_like(P), torch.empty_like(P), torch.empty_like(P)
    dev.cv_terms(P, 1.0, 1.0, 0.06, H, G)
    if kernels_only:
        dev.cv_solver(P, Dd, H, G, 0.5, 0.3, o)
        torch.cuda.synchronize()
    else:
        res["cv_solver_2160x3840x1_us"] = timed(lambda: dev.cv_solver(P, Dd, H, G, 0.5, 0.3, o), reps)
    return res


def _kernel_split(outdir):
    """Per-kernel average durations (us) and call counts from rocprofv3's kernel stats CSV."""
    split = {}
    for path in glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row.get("Name", "")
                for key in KERNELS:
                    if key in name:
                        split[key + "_us"] = float(row["AverageNs"]) / 1e3
                        split[key + "_calls"] = int(row["Calls"])
    return split


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
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
                               "-o", "diffusion", "--", sys.executable, me, "--child", "kernels"],
                              capture_output=True, text=True, cwd=ROOT)
        if step.returncode != 0:
            res["rocprof_error"] = "rocprofv3 step exited %d: %s" % (step.returncode, step.stderr[-400:])
        else:
            split = _kernel_split(tmp)
            if "k_diff4_lines_us" in split and "k_cv_lines_us" in split:
                split["lines_ratio"] = split["k_diff4_lines_us"] / split["k_cv_lines_us"]
            res["kernel_split_2160x3840x1"] = split
    print(json.dumps(res))
    if "rocprof_error" in res:
        sys.exit(1)


if __name__ == "__main__":
    main()
