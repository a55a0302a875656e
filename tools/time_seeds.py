"""Time connected-component labelling, generateSeeds() and DispSegmentation on one GPU; prints one JSON line.

    python tools/time_seeds.py [--reps N] [--skip-restatement]

The parent process never touches the GPU.  It runs two child steps, each under its own time limit (nothing is retried; the second
is not started if the first fails):
  pdeip_bwlabel_dev (labels, num and the areas) at 58x77 (the coarse pyramid scale the drivers label at, for a 288x384 map),
  288x384 and 2160x3840, in the one-workgroup form and the tiled form where both apply (PDEIP_CCL_SMALL), conn 8, on a random
  0.55-density mask and on the one-pixel-wide serpentine of the tests (tests/ccl_cases.py): us per call (a host clock around
  `reps` calls that end in a device synchronise) and the achieved GB/s of 8 B/pixel (the mask in, the labels out).  Every result is
  compared with the flood fill of tests/ccl_ref.py first (at 2160x3840: num and the areas against scipy.ndimage.label, which the
  flood fill is pinned to), so a time is never reported for a wrong answer.
  one drivers.generateSeeds (polyorder 1, sigmaLim 0.7, the driver's cset_vect, 20 iterations, 15 seeds, gen_scl 0.2) and one
  drivers.DispSegmentation with the defaults on a 288x384 map of three noisy planes (tests/seeds_cases.three_planes): seconds per
  call after one warm-up call, and S.  Beside each the time of the NumPy restatement (tests/seeds_ref.py) on the same input -- a
  checker, not a baseline; it takes many minutes at this size, --skip-restatement leaves it out.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
SHAPES = [(58, 77), (288, 384), (2160, 3840)]
DENSITY = 0.55


def _child(reps):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import importlib

    import numpy as np
    import torch
    from scipy import ndimage

    import ccl_cases
    import ccl_ref

    dev = importlib.import_module("pde-based-image-processing_amd.device")
    res = {}
    for nr, nc in SHAPES:
        masks = {"random": (np.random.default_rng(nr).random((nr, nc)) < DENSITY).astype(np.float32),
                 "serpentine": ccl_cases.serpentine(nr, nc).astype(np.float32)}
        for kind, A in masks.items():
            if nr * nc <= 1 << 18:
                wL, wnum, wareas = ccl_ref.label(A, 8)
            else:
                lab, wnum = ndimage.label((A > 0).T, structure=np.ones((3, 3), int))
                wL, wareas = lab.T, np.bincount(lab.ravel(), minlength=wnum + 1)[1:]
            tA = dev.to_device(np.asfortranarray(A))
            L = torch.empty(tA.shape, dtype=torch.int32, device="cuda")
            num = torch.empty(1, dtype=torch.int32, device="cuda")
            areas = torch.empty(max(wnum, 1), dtype=torch.int32, device="cuda")
            for small in ((1, 0) if ccl_cases.admits_small(A) else (0,)):
                os.environ["PDEIP_CCL_SMALL"] = str(small)

                def call():
                    dev.bwlabel(tA, 8, L, num, areas)

                call()
                torch.cuda.synchronize()
                if int(num.item()) != wnum or not np.array_equal(L.cpu().numpy().T, wL) or not np.array_equal(areas.cpu().numpy()[:wnum], wareas):
                    raise AssertionError("bwlabel differs from the reference at %dx%d %s small=%d" % (nr, nc, kind, small))
                n = reps if nr * nc < 1 << 20 else max(reps // 10, 5)
                t0 = time.perf_counter()
                for _ in range(n):
                    call()
                torch.cuda.synchronize()
                us = (time.perf_counter() - t0) / n * 1e6
                res["%dx%d_%s_%s" % (nr, nc, kind, "small" if small else "tiled")] = {
                    "us": round(us, 2), "GBps": round(8.0 * nr * nc / us / 1e3, 2), "num": wnum, "reps": n}
    os.environ.pop("PDEIP_CCL_SMALL", None)
    print(json.dumps({"bwlabel_dev": res, "device": torch.cuda.get_device_name(0)}))


def _child_drivers(restate):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import importlib

    import seeds_cases
    import seeds_ref

    drv = importlib.import_module("pde-based-image-processing_amd.drivers")
    D = seeds_cases.three_planes(288, 384, 1)[0]
    cset = seeds_ref.cset_vector(0.1, 0.7, 10)
    res = {}

    def timed(fn, warm):
        if warm:
            fn()
        t0 = time.perf_counter()
        out = fn()
        return out, round(time.perf_counter() - t0, 4)

    (PHI, _), t = timed(lambda: drv.generateSeeds(D, 1, 0.7, cset, 20, seeds=15, seed=1), True)
    res["generateSeeds_288x384"] = {"s": t, "S": int(PHI.shape[2])}
    (PHI, _, _), t = timed(lambda: drv.DispSegmentation(D, seed=1), True)
    res["DispSegmentation_288x384"] = {"s": t, "S": int(PHI.shape[2])}
    if restate:
        out, t = timed(lambda: seeds_ref.generate_seeds(D, 1, 0.7, cset, 20, seeds=15, pyr_scl=0.2, seed=1), False)
        res["generateSeeds_288x384"].update(restatement_s=t, restatement_S=out["S"])
        out, t = timed(lambda: seeds_ref.disp_segmentation(D, seed=1), False)
        res["DispSegmentation_288x384"].update(restatement_s=t, restatement_S=out["S"])
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--skip-restatement", action="store_true")
    ap.add_argument("--child", choices=("bwlabel", "drivers"))
    a = ap.parse_args()
    if a.child == "bwlabel":
        return _child(a.reps)
    if a.child == "drivers":
        return _child_drivers(not a.skip_restatement)
    me = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps)] + (["--skip-restatement"] if a.skip_restatement else [])
    result = {}
    for step, limit in (("bwlabel", 420), ("drivers", 420 if a.skip_restatement else 7200)):
        out = subprocess.run(me + ["--child", step], capture_output=True, text=True, cwd=ROOT, timeout=limit)
        if out.returncode != 0:
            sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
            return out.returncode
        result.update(json.loads(out.stdout.strip().splitlines()[-1]))
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
