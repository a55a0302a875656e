"""Time region competition (one level of the segmentation drivers' inner loop) on one GPU; prints one JSON line.

    python tools/time_segmentation.py [--reps N]

The parent process never touches the GPU.  It runs two child steps, each under its own time limit, and stops at the first
that fails (nothing is retried):
  1. timing: ms per pdeip_seg_competition_level_dev call of 30 iterations at 115x154x15 and 288x384x15 (the drivers' rc_scl
     scale and full scale), dense `inverse`, orders 1 and 2, no segment removed, and the wall time of the fit stage of one odd
     iteration, each in both forms -- `batched` (one pdeip_surface_fit_masked_batch_dev call, the default) and `chained` (one
     pdeip_surface_fit_masked_dev chain per segment, PDEIP_SEG_FIT_CHAINS=1: the form before the batch call existed and the
     baseline) -- alternated --ab times in this one process on this one device; a sample is the mean of --reps calls enqueued
     back to back and synchronised once, as the level enqueues them.  Reported per form: median, min and max of the samples.
     `batched_wins` holds where the chained median exceeds the batched one by more than the spread (the larger max - min of
     the two forms).  Beside it an even iteration's sizes + read-back + Chan-Vese step (even_us), from which per form odd_us =
     (level - 15*even_us)/15 and fit_share = fit_us/odd_us; and the NumPy restatement (tests/segmentation_ref.py) of the same
     level on the host, timed on 2 iterations and scaled to 30 (ref_ms, an extrapolation; the restatement is a checker, not a
     baseline);
  2. `rocprofv3 --kernel-trace --stats` of one 288x384x15 order-1 level (the default form): calls and total us per kernel.
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
SHAPES = [(115, 154), (288, 384)]
SEGMENTS, ITERATIONS, REF_ITERATIONS = 15, 30, 2
KERNELS = ("k_seg_sizes_final", "k_seg_sizes", "k_seg_variance_final", "k_seg_variance", "k_seg_data", "k_cv_terms", "k_cv_lines", "k_cv_combine",
           "k_mask_count", "k_mask_scan", "k_mask_scatter", "k_ransac_fit", "k_ransac_score", "k_ransac_select", "k_ransac_dist", "k_copy_d2d")
FIT_KERNELS = KERNELS[KERNELS.index("k_mask_count"):KERNELS.index("k_copy_d2d")]
FORMS = ("batched", "chained")
SWITCH = "PDEIP_SEG_FIT_CHAINS"


def _inputs(nr, nc):
    """A disparity map of 3 x 5 tiles, each its own plane, and one box-shaped segment inside each tile."""
    import numpy as np

    rng = np.random.default_rng(3)
    jj, ii = np.meshgrid(np.arange(nc) + 1.0, np.arange(nr) + 1.0)
    D = np.zeros((nr, nc))
    PHI = -np.ones((nr, nc, SEGMENTS), np.float32)
    for k in range(SEGMENTS):
        r, c = divmod(k, 5)
        r0, r1, c0, c1 = r * nr // 3, (r + 1) * nr // 3, c * nc // 5, (c + 1) * nc // 5
        D[r0:r1, c0:c1] = (8.0 * k + 0.03 * (k % 4 - 1.5) * jj + 0.02 * (k % 3 - 1) * ii)[r0:r1, c0:c1]
        mr, mc = (r1 - r0) // 5, (c1 - c0) // 5
        PHI[r0 + mr:r1 - mr, c0 + mc:c1 - mc, k] = 1
    D += rng.normal(0, 0.05, D.shape)
    return np.asfortranarray(D.astype(np.float32)), np.asfortranarray(PHI)


def _stats(samples):
    import statistics

    return {"median": statistics.median(samples), "min": min(samples), "max": max(samples), "n": len(samples)}


def _child_timing(reps, kernels_only, ab=5):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import importlib

    import numpy as np
    import torch

    import segmentation_ref as sr

    dev = importlib.import_module("pde-based-image-processing_amd.device")

    def wall(fn, n):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    res = {}
    cases = [(288, 384, 1)] if kernels_only else [(nr, nc, o) for nr, nc in SHAPES for o in (1, 2)]
    for nr, nc, order in cases:
        D, PHI = _inputs(nr, nc)
        P = torch.from_numpy(np.ascontiguousarray(PHI.transpose(2, 1, 0))).cuda()
        Dd = dev.to_device(D)
        S_out = []

        def level():
            out = dev.seg_competition_level(P, Dd, order, 1.5, 0.7, ITERATIONS, 0.0, "inverse", seed=1)
            S_out.append(len(out[2]))

        if kernels_only:
            level()
            torch.cuda.synchronize()
            continue
        M = torch.zeros((SEGMENTS, 3 if order == 1 else 6), dtype=torch.float32, device="cuda")
        dist, DATA, DH, G, nxt = (torch.empty_like(P) for _ in range(5))
        sizes = torch.zeros(SEGMENTS, dtype=torch.int32, device="cuda")

        def fits_chained():
            for k in range(SEGMENTS):
                dev.surface_fit_masked(P[k], Dd, order, M[k], 1.0, 0.7, 10, M[k], dist[k], None, seed=k)

        def fits_batched():
            dev.surface_fit_masked_batch(P, Dd, order, M, 1.0, 0.7, 10, M, dist, None, seed=0, seed_stride=1)

        fits = {"batched": fits_batched, "chained": fits_chained}
        fit_us, level_ms = {f: [] for f in FORMS}, {f: [] for f in FORMS}
        for _ in range(ab):  # the two forms in turn, so that a drift of the device or the host falls on both
            for form in FORMS:
                M.zero_()
                fit_us[form].append(wall(fits[form], reps) * 1e6)
                os.environ.pop(SWITCH, None)
                if form == "chained":
                    os.environ[SWITCH] = "1"
                try:
                    level_ms[form].append(wall(level, reps) * 1e3)
                finally:
                    os.environ.pop(SWITCH, None)
        r = {"S_out": S_out[-1], "fit_us": {f: _stats(fit_us[f]) for f in FORMS}, "level_ms": {f: _stats(level_ms[f]) for f in FORMS}}
        spread = max(r["fit_us"][f]["max"] - r["fit_us"][f]["min"] for f in FORMS)
        r["fit_us"]["spread"] = spread
        r["batched_wins"] = r["fit_us"]["chained"]["median"] - r["fit_us"]["batched"]["median"] > spread

        def even():
            dev.seg_sizes(P, sizes)
            sizes.cpu()
            dev.cv_solver(P, DATA, DH, G, 1.0, 0.3, nxt)

        dev.cv_terms(P, 1.0, 1.0, 0.06, DH, G)
        DATA.zero_()
        r["even_us"] = wall(even, reps) * 1e6
        r["odd_us"] = {f: (r["level_ms"][f]["median"] * 1e3 - (ITERATIONS // 2) * r["even_us"]) / (ITERATIONS - ITERATIONS // 2) for f in FORMS}
        r["fit_share"] = {f: r["fit_us"][f]["median"] / r["odd_us"][f] for f in FORMS}
        t0 = time.perf_counter()
        sr.level(PHI, D, order, sr.INVERSE, 1.5, 0.7, REF_ITERATIONS, 0.0, seed=1)
        r["ref_ms"] = (time.perf_counter() - t0) * 1e3 * ITERATIONS / REF_ITERATIONS
        res["%dx%dx%d_o%d" % (nr, nc, SEGMENTS, order)] = r
    return res


def _kernel_split(outdir):
    """Calls and total duration (us) per kernel from rocprofv3's kernel stats CSV; the fit chains' share of the GPU time."""
    split, total, fit = {}, 0.0, 0.0
    for path in glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row.get("Name", "")
                us = float(row["TotalDurationNs"]) / 1e3
                total += us
                for key in KERNELS:  # the *_final names come first: they contain the plain ones
                    if key in name:
                        e = split.setdefault(key, {"calls": 0, "total_us": 0.0})
                        e["calls"] += int(row["Calls"])
                        e["total_us"] += us
                        if key in FIT_KERNELS:
                            fit += us
                        break
    split["all_kernels_us"] = total
    split["fit_chain_share_of_gpu_time"] = fit / total if total else None
    return split


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ab", type=int, default=5, help="alternations of the batched and the chained form (at least 5)")
    ap.add_argument("--child", choices=["full", "kernels"])
    a = ap.parse_args()
    if a.child:
        print(json.dumps(_child_timing(a.reps, a.child == "kernels", max(a.ab, 5))))
        return
    res = {}
    me = os.path.abspath(__file__)
    step = subprocess.run(["timeout", "-k", "10", "300", sys.executable, me, "--child", "full", "--reps", str(a.reps), "--ab", str(a.ab)],
                          capture_output=True, text=True, cwd=ROOT)
    if step.returncode != 0:
        res["error"] = "timing step exited %d: %s" % (step.returncode, step.stderr[-400:])
        print(json.dumps(res))
        sys.exit(1)
    res.update(json.loads(step.stdout.strip().splitlines()[-1]))
    with tempfile.TemporaryDirectory() as tmp:
        step = subprocess.run(["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp,
                               "-o", "segmentation", "--", sys.executable, me, "--child", "kernels"],
                              capture_output=True, text=True, cwd=ROOT)
        if step.returncode != 0:
            res["rocprof_error"] = "rocprofv3 step exited %d: %s" % (step.returncode, step.stderr[-400:])
        else:
            res["kernel_split_288x384x15_o1"] = _kernel_split(tmp)
    print(json.dumps(res))
    if "rocprof_error" in res:
        sys.exit(1)


if __name__ == "__main__":
    main()
