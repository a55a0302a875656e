"""Line relaxation (solver = 2) in the reference's line order: EXACT_ORDER (k_alr_lex) against LINE_SCAN (k_alr_scan) on device
pointers.  The two modes alternate on one card, three runs each; per run the wall time of one call between two device
synchronisations.  Reports microseconds per iteration and per line step (an iteration walks ncols + nrows line steps; the two
fields of a coupled model share a step), the RMS / max-abs distance of the two results, and one JSON line at the end.

    python tools/time_line_scan.py [--quick | --4k]        (--quick: the 388 x 584 shape only; --4k: the 2160 x 3840 elin4 shape only)
"""
import json, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import numpy as np
import torch
from pdeip_amd import capi, device as dev
import problems as pb

SHAPES = [  # name, entry point, problem, iterate planes, iter, omega
    ("elin4 2160x3840", dev.oflow_alr_elin4, lambda: pb.elin4(7, 2160, 3840), ("U", "V"), 4, 1.9),
    ("llin4 1080x1920", dev.oflow_alr_llin4, lambda: pb.llin4(7, 1080, 1920), ("dU", "dV"), 4, 1.4),
    ("pde4 2160x3840 F=1", dev.pde_alr4, lambda: pb.pde4(7, 2160, 3840), ("X",), 4, 1.3),
    ("elin4 388x584", dev.oflow_alr_elin4, lambda: pb.elin4(7, 388, 584), ("U", "V"), 20, 1.9),
]


def one(fn, p, names, it, omega, mode):
    d = {k: dev.to_device(v) for k, v in p.items()}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(*d.values(), it, omega, mode)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, [dev.to_matlab(d[k]) for k in names]


def main():
    results = []
    for name, fn, make, names, it, omega in SHAPES[-1:] if "--quick" in sys.argv else (SHAPES[:1] if "--4k" in sys.argv else SHAPES):
        p = make()
        nr, nc = p[names[0]].shape[:2]
        one(fn, p, names, 1, omega, capi.MODE_LINE_SCAN)  # workspaces, code objects
        one(fn, p, names, 1, omega, capi.MODE_EXACT_ORDER)
        t = {capi.MODE_EXACT_ORDER: [], capi.MODE_LINE_SCAN: []}
        out = {}
        for _ in range(3):
            for mode in (capi.MODE_EXACT_ORDER, capi.MODE_LINE_SCAN):
                dt, out[mode] = one(fn, p, names, it, omega, mode)
                t[mode].append(dt)
        diff = [np.asarray(a, np.float64) - np.asarray(b, np.float64) for a, b in zip(out[capi.MODE_LINE_SCAN], out[capi.MODE_EXACT_ORDER])]
        rms, mx = max(float(np.sqrt(np.mean(d * d))) for d in diff), max(float(np.max(np.abs(d))) for d in diff)
        row = dict(shape=name, iter=it, omega=omega, rms=rms, maxabs=mx)
        for mode, key in ((capi.MODE_EXACT_ORDER, "exact"), (capi.MODE_LINE_SCAN, "scan")):
            best = min(t[mode])
            row[key] = dict(ms_per_call=[round(x * 1e3, 3) for x in t[mode]], us_per_iter=best / it * 1e6, us_per_line=best / it / (nr + nc) * 1e6,
                            iter_per_s=it / best)
            print("%-20s %-6s %9.1f us/iteration %7.2f us/line step %8.2f it/s   calls (ms): %s" %
                  (name, key, row[key]["us_per_iter"], row[key]["us_per_line"], row[key]["iter_per_s"], row[key]["ms_per_call"]), flush=True)
        row["speedup"] = row["scan"]["iter_per_s"] / row["exact"]["iter_per_s"]
        print("%-20s scan / exact = %.2fx   rms %.3g  max-abs %.3g" % (name, row["speedup"], rms, mx), flush=True)
        results.append(row)
    print(json.dumps(dict(tool="time_line_scan", results=results)))


if __name__ == "__main__":
    main()
