"""Time the level-set path on one GPU; prints one JSON line.

    python tools/time_levelset.py [--reps N]

The parent process never touches the GPU.  It runs two child steps, each under its own time limit, and stops at the first
that fails (nothing is retried):
  1. timing: us per AC_solver_2d and per Reinit(T=10) call at 2160x3840 on device pointers (eager and graph-replayed), ms per
     GAC_v10a / GAC_v10b call on drivsco image 1 (eager and graph-replayed), the numpy restatement's time (the checker,
     labelled as such: not the reference's C);
  2. `rocprofv3 --kernel-trace --stats` of the 4K AC_solver_2d / Reinit calls: the column-pass / row-pass / re-initialisation
     split per kernel.
and adds the bytes model (two passes ~116 B/px as built, 52 B/px minimum; 8 B/px per re-initialisation step) and the
chain-latency model (~40 cycles per line element at 2.4 GHz) of DESIGN.md section 5.7.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NR, NC = 2160, 3840
HBM_BPS = 5.3e12


def _child_timing(reps, kernels_only):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import ctypes
    import importlib

    import numpy as np
    import torch

    dev = importlib.import_module("pde-based-image-processing_amd.device")
    capi = importlib.import_module("pde-based-image-processing_amd.capi")
    drivers = importlib.import_module("pde-based-image-processing_amd.drivers")

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
    host = [rng.uniform(-3, 3, (NR, NC)), rng.uniform(-1, 1, (NR, NC)), rng.uniform(0, 1.5, (NR, NC)), rng.uniform(0.1, 2, (NR, NC))]
    host = [np.asfortranarray(x.astype(np.float32)) for x in host]
    P, D, G, Df = (dev.to_device(x) for x in host)
    out, r = torch.empty_like(P), torch.empty_like(P)
    res = {}
    res["ac_solver_us"] = timed(lambda: dev.ac_solver(P, D, G, Df, 0.25, 1.0, out), reps)
    res["reinit_T10_us"] = timed(lambda: dev.reinit(P, 10.0, r), reps)
    if kernels_only:
        return res
    res["ac_solver_graph_us"] = graphed(lambda: dev.ac_solver(P, D, G, Df, 0.25, 1.0, out), reps)
    res["reinit_T10_graph_us"] = graphed(lambda: dev.reinit(P, 10.0, r), reps)
    z = np.load(os.path.join(ROOT, "tests", "golden", "levelset", "drivsco.npz"))
    I1 = np.asfortranarray(z["I1"].astype(np.float32) / np.float32(255))
    PHI = -np.ones(I1.shape[:2], np.float32, order="F")
    PHI[41:175, 114:217] = 1
    dI, dP = dev.to_device(I1), dev.to_device(PHI)
    g_out = torch.empty_like(dP)
    prm = drivers._GacParams(*([float("nan")] * 5))
    for model, name in ((0, "gac_v10a"), (1, "gac_v10b")):
        call = lambda: capi.call("pdeip_gac_dev", dev._stream(), dI.data_ptr(), PHI.shape[0], PHI.shape[1], 3, dP.data_ptr(), model,  # noqa: E731
                                 ctypes.addressof(prm), g_out.data_ptr())
        res[name + "_ms"] = timed(call, 3) / 1e3
        res[name + "_graph_ms"] = graphed(call, 3) / 1e3
        t0 = time.time()
        (drivers.GAC_v10a if model == 0 else drivers.GAC_v10b)(I1, PHI)
        res[name + "_host_call_ms"] = (time.time() - t0) * 1e3  # upload + run + download
    import levelset_ref as ref

    t0 = time.time()
    ref.AC_solver_2d(*host, 0.25, 1.0)
    res["numpy_restatement_ac_solver_s"] = time.time() - t0
    t0 = time.time()
    ref.GAC(I1, PHI, "a")
    res["numpy_restatement_gac_v10a_s"] = time.time() - t0
    return res


def _kernel_split(outdir):
    """Per-kernel average durations (us) from rocprofv3's kernel stats CSV."""
    split = {}
    for path in glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row.get("Name", "")
                for key, label in (("k_aos_col", "column_pass_us"), ("k_aos_row", "row_pass_us"), ("k_reinit_step", "reinit_step_us")):
                    if key in name:
                        split[label] = float(row["AverageNs"]) / 1e3
    return split


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--child", choices=["full", "kernels"])
    a = ap.parse_args()
    if a.child:
        print(json.dumps(_child_timing(a.reps, a.child == "kernels")))
        return
    res = {"shape": [NR, NC]}
    me = os.path.abspath(__file__)
    step = subprocess.run(["timeout", "-k", "10", "900", sys.executable, me, "--child", "full", "--reps", str(a.reps)],
                          capture_output=True, text=True, cwd=ROOT)
    if step.returncode != 0:
        res["error"] = "timing step exited %d: %s" % (step.returncode, step.stderr[-400:])
        print(json.dumps(res))
        sys.exit(1)
    res.update(json.loads(step.stdout.strip().splitlines()[-1]))
    with tempfile.TemporaryDirectory() as tmp:
        step = subprocess.run(["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp,
                               "-o", "ls", "--", sys.executable, me, "--child", "kernels", "--reps", "5"],
                              capture_output=True, text=True, cwd=ROOT)
        if step.returncode != 0:
            res["rocprof_error"] = "rocprofv3 step exited %d: %s" % (step.returncode, step.stderr[-400:])
        else:
            res["kernel_split"] = _kernel_split(tmp)
    px = NR * NC
    res["ac_bytes_model_us"] = 116 * px / HBM_BPS * 1e6
    res["ac_min_bytes_model_us"] = 52 * px / HBM_BPS * 1e6
    res["reinit_step_bytes_model_us"] = 8 * px / HBM_BPS * 1e6
    res["chain_model_us"] = {"column_pass": NR * 40 / 2.4e9 * 1e6, "row_pass": NC * 40 / 2.4e9 * 1e6}
    print(json.dumps(res))
    if "rocprof_error" in res:
        sys.exit(1)


if __name__ == "__main__":
    main()
