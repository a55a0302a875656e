"""Time the structure-tensor diffusion calls (csrc/pdeip_stensor.hip) on one GPU; prints one JSON line.

    python tools/time_stensor.py [--reps N] [--order 0|1]

The parent process never touches the GPU.  It runs two child steps, each under its own time limit, and stops at the first
that fails (nothing is retried):
  1. timing, at 320x400x3, 1080x1920x3 and 2160x3840x1: us per call on device pointers of gaussian at sigma 1.25, 4 and 10 (with
     the bytes the two passes must move, 16 per pixel and frame, and the rate that gives), of fas_gauss5 on the same plane in the
     same process (the 25-tap direct filter: the same 8 bytes per pixel and frame in one pass), of structure_tensor and st_weights_padded
     at the CED defaults, and of diffusion8 in both modes with both solvers, eager and graph-replayed, in the ordering --order
     (default 1, red-black / zebra: the parallel one; 0, the reference's order, is timed eagerly only);
  2. `rocprofv3 --kernel-trace --stats` of one CED point-SOR diffusion8 call at 2160x3840x1: the new kernels' us, and their share
     of the call against the solver's kernels.
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
SHAPES = [(320, 400, 3), (1080, 1920, 3), (2160, 3840, 1)]
NEW_KERNELS = ("k_gauss_rows", "k_gauss_cols", "k_st_products", "k_st_weights", "k_st_pad", "k_st_crop")


def _image(rng, shape):
    import numpy as np

    blocks = rng.uniform(0, 255, (shape[0] // 16 + 1, shape[1] // 16 + 1) + tuple(shape[2:]))
    I = blocks[np.arange(shape[0]) // 16][:, np.arange(shape[1]) // 16] + rng.normal(0, 6, shape)
    return np.asfortranarray(np.clip(I, 0, 255).astype(np.float32))


def _child_timing(reps, order, kernels_only):
    sys.path.insert(0, ROOT)
    import importlib

    import numpy as np
    import torch

    pkg = importlib.import_module("pde-based-image-processing_amd")
    dev = importlib.import_module("pde-based-image-processing_amd.device")
    pyramid = importlib.import_module("pde-based-image-processing_amd.pyramid")
    pkg.capi.set_mode(order)

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
    res = {"order": order}
    for nr, nc, nf in (SHAPES[-1:] if kernels_only else SHAPES):
        I = dev.to_device(_image(rng, (nr, nc, nf) if nf > 1 else (nr, nc)))
        planes = I if I.dim() == 3 else I[None]
        out = torch.empty_like(I)
        ced = dev.diffusion8_params("ced")
        if kernels_only:
            dev.diffusion8(I, ced, out)
            dev.diffusion8(I, ced, out)
            torch.cuda.synchronize()
            continue
        r = {}
        for sigma in (1.25, 4.0, 10.0):
            us = timed(lambda: dev.gaussian(I, sigma, out), reps)
            nbytes = 16.0 * nr * nc * nf   # each pass reads and writes every element once
            r["gauss_sigma%g" % sigma] = {"us": us, "bytes": nbytes, "GBps": nbytes / us / 1e3}
        G = pyramid.gaussian5(1.25)
        us = timed(lambda: dev.fas_gauss5(planes, G), reps)
        r["fas_gauss5"] = {"us": us, "bytes": 8.0 * nr * nc * nf, "GBps": 8.0 * nr * nc * nf / us / 1e3}
        J = torch.empty((3, nc, nr), dtype=torch.float32, device=I.device)
        TRACE = torch.empty((nc + 2, nr + 2), dtype=torch.float32, device=I.device)
        w8 = torch.empty((8, nc + 2, nr + 2), dtype=torch.float32, device=I.device)
        r["structure_tensor_us"] = timed(lambda: dev.structure_tensor(planes, 0.7, 4.0, J), reps)
        r["st_weights_padded_us"] = timed(lambda: dev.st_weights_padded(J, ced, 1.0, TRACE, w8), reps)
        r["st_weights_padded_bytes"] = 4.0 * (3 * nr * nc + 9 * (nr + 2) * (nc + 2))
        for mode in ("ced", "eed"):
            for solver in (1, 2):
                prm = dev.diffusion8_params(mode, solver=solver)
                key = "diffusion8_%s_solver%d" % (mode, solver)
                r[key + "_us"] = timed(lambda: dev.diffusion8(I, prm, out), max(reps // 4, 2))
                if order != 0:   # the exact-order solvers are timed eagerly only
                    r[key + "_graph_us"] = graphed(lambda: dev.diffusion8(I, prm, out), max(reps // 4, 2))
        res["%dx%dx%d" % (nr, nc, nf)] = r
    dev.sync_check()
    return res


def _kernel_split(outdir):
    """Per-kernel average durations (us), call counts and the new kernels' share of all kernel time from rocprofv3's stats CSV."""
    split, new_ns, all_ns = {}, 0.0, 0.0
    for path in glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row.get("Name", "")
                total = float(row["AverageNs"]) * int(row["Calls"])
                all_ns += total
                for key in NEW_KERNELS:
                    if key in name:
                        split[key + "_us"] = float(row["AverageNs"]) / 1e3
                        split[key + "_calls"] = int(row["Calls"])
                        new_ns += total
    if all_ns > 0:
        split["new_kernels_share"] = new_ns / all_ns
        split["all_kernels_ms"] = all_ns / 1e6
    return split


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--order", type=int, default=1)
    ap.add_argument("--child", choices=["full", "kernels"])
    a = ap.parse_args()
    if a.child:
        print(json.dumps(_child_timing(a.reps, a.order, a.child == "kernels")))
        return
    res = {}
    me = os.path.abspath(__file__)
    step = subprocess.run(["timeout", "-k", "10", "600", sys.executable, me, "--child", "full", "--reps", str(a.reps), "--order", str(a.order)],
                          capture_output=True, text=True, cwd=ROOT)
    if step.returncode != 0:
        res["error"] = "timing step exited %d: %s" % (step.returncode, step.stderr[-400:])
        print(json.dumps(res))
        sys.exit(1)
    res.update(json.loads(step.stdout.strip().splitlines()[-1]))
    with tempfile.TemporaryDirectory() as tmp:
        step = subprocess.run(["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp,
                               "-o", "stensor", "--", sys.executable, me, "--child", "kernels", "--order", str(a.order)],
                              capture_output=True, text=True, cwd=ROOT)
        if step.returncode != 0:
            res["rocprof_error"] = "rocprofv3 step exited %d: %s" % (step.returncode, step.stderr[-400:])
        else:
            res["kernel_split_ced_2160x3840x1"] = _kernel_split(tmp)
    print(json.dumps(res))
    if "rocprof_error" in res:
        sys.exit(1)


if __name__ == "__main__":
    main()
