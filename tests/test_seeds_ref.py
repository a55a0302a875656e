"""CPU: the fixtures of the generateSeeds() / DispSegmentation tests (seeds_cases.py) and their restatement (seeds_ref.py).  Fixes
what the GPU test compares exactly and proves that no fixture decides anything on a knife's edge: with DRIFT the measured change
of PHI under a one-ulp perturbation of DATA, every `>= 0` / `> 0` decision on PHI and every `AA > 0.05` decision clears DRIFT
tenfold, every count differs from 20 by at least 3 pixels, the largest component beats the second by at least 3 pixels, and every
RANSAC `sum < best` comparison has a relative margin of at least 1e-3."""
import functools

import numpy as np
import pytest

import seeds_cases as sc
import seeds_ref as gs
import segmentation_ref as sr

ALL = sorted(sc.SEEDS_CASES) + sorted(sc.DRIVER_CASES)


def _iters(trace):
    return [r for r in trace if "PHI" in r]


def _decisions(out, trace):
    """What must not change under the perturbation: counts, EMPTY decisions, removals, the largest-component planes, the models."""
    d = [out["S"], out["surf"].tobytes()]
    for r in trace:
        if "largest" in r:
            d.append(r["largest"].tobytes())
        elif "count" in r:
            d.append(r["count"])
        else:
            d.append((tuple(int(x) for x in r["sizes"]), tuple(r["removed"])))
        if "PHI" in r:
            d.append(sr.mask(r["PHI"]).tobytes())
    return d


@functools.lru_cache(maxsize=None)
def measured_drift(name):
    out, trace = sc.run(name)
    pout, ptrace = sc.run(name, perturbed=True)
    assert _decisions(out, trace) == _decisions(pout, ptrace), "%s: the perturbation changed a decision" % name
    drift = 0.0
    for a, b in zip(_iters(trace), _iters(ptrace)):
        drift = max(drift, float(np.max(np.abs(a["PHI"].astype(np.float64) - b["PHI"]))))
    if out["S"]:
        drift = max(drift, float(np.max(np.abs(out["PHI"].astype(np.float64) - pout["PHI"]))))
    return drift


def margins(out, trace):
    m = dict(count=np.inf, phi=np.inf, aa=np.inf, ransac=np.inf, component=np.inf, size=np.inf)
    for r in trace:
        if "largest" in r:
            a = [int(x) for x in r["areas"]] + [0]
            if a[0] > 0:
                m["component"] = min(m["component"], a[0] - a[1])
            m["phi"] = min(m["phi"], r["min_phi"])
            continue
        m["ransac"] = min(m["ransac"], r["min_ransac"])
        if "count" in r:
            m["count"] = min(m["count"], abs(r["count"] - 20))
            m["aa"] = min(m["aa"], r["min_aa"])
            if r["count"] >= 20:
                m["phi"] = min(m["phi"], r["min_phi"])
        else:
            m["phi"] = min(m["phi"], r["min_phi"])
            m["size"] = min(m["size"], r["min_size"])
    if out["S"]:
        m["phi"] = min(m["phi"], float(np.min(np.abs(out["PHI"]))))
    return m


@pytest.mark.parametrize("name", ALL)
def test_drift_and_decision_margins(name):
    drift = measured_drift(name)
    out, trace = sc.run(name)
    m = margins(out, trace)
    rec = sc.DRIFT[name]
    print("%s: drift %.3g (recorded %.3g); margins %r" % (name, drift, rec, m))
    assert drift <= rec, "DRIFT[%r] = %g is smaller than the measured %g" % (name, rec, drift)
    assert rec <= 2 * drift + 1e-12, "DRIFT[%r] = %g is not the measured value (%g)" % (name, rec, drift)
    assert m["phi"] > 10 * rec and m["aa"] > 10 * rec
    assert m["count"] >= 3 and m["size"] >= 3
    assert m["component"] >= 3
    assert m["ransac"] >= 1e-3


def test_fixtures_are_what_they_claim():
    for order in (1, 2):
        out, trace = sc.run("planes60x80_o%d" % order)
        assert out["sizes"] == [(60, 80), (42, 56), (30, 40)] and out["surf"].shape[0] == (3, 6)[order - 1]
        assert {r["visit"] for r in trace} == set(range(6)) and max(r["iter"] for r in _iters(trace)) == 8
        assert 1 <= out["S"] <= 4
    a = sc.SEEDS_CASES["sparse37x53"]()
    assert np.isnan(a["D"]).any() and a["prm"] == gs.SPARSE
    out, trace = sc.run("tiny_aa")
    assert out["S"] == 0 and out["fit_counter"] == 0 and [r["count"] for r in trace] == [1, 1, 1]
    assert out["gamma"] == 0.01 * 0.8 * 0.8 * 0.8
    out, trace = sc.run("used_up")
    counts = {}
    for r in trace:
        if "count" in r:
            counts.setdefault(r["seed"], []).append(r["count"])
    assert out["S"] == 1 and min(counts[0]) >= 20 and all(counts[s] == [counts[s][0]] and counts[s][0] < 20 for s in (1, 2))
    a = sc.SEEDS_CASES["short_cset"]()
    assert len(a["cset_vect"]) < a["iterations"]
    for name in ("short_cset", "short_cset_o2"):
        _, trace = sc.run(name)
        assert min(r["min_ransac"] for r in _iters(trace)) < np.inf  # these fixtures do compare sums
    out, trace = sc.run("zero_iterations")
    assert out["S"] == 2 and out["fit_counter"] == 0 and np.isnan(out["surf"]).all() and not _iters(trace)
    band, _ = sc.run("band60x80")
    assert band["S"] >= 1 and (band["PHI"][:, 31:43, :] < 0).all()  # nothing grows into the excluded band


def test_schedule():
    cset = [0.1, 0.2, 0.3]
    assert [gs.visit_scale(v, 3) for v in range(6)] == [0, 1, 2, 2, 1, 0]
    assert gs.riter(1, 0) == 2000 and gs.riter(2, 0) == 100 and gs.riter(1, 1) == 100
    assert [gs.rcons(cset, it, 0) for it in (1, 2, 3, 4, 9)] == [0.1, 0.2, 0.3, 0.3, 0.3]
    assert gs.rcons(cset, 1, 1) == 0.3
    P = gs.initial_phi(12, 13)
    assert (np.argwhere(P > 0) == [[i, j] for i in (1, 6) for j in (1, 6, 11)]).all()  # rows <= 10, columns <= 11


def test_driver_branches():
    one, t1 = sc.run("driver_seeds1")
    assert one["stages"] == 1 and one["S"] == 1 and {r["kind"] for r in t1} == {"seeds"}
    three, t3 = sc.run("driver_seeds3")
    assert three["stages"] == 4 and [k for k, _ in _runs(t3)] == ["seeds", "rc", "seeds", "rc"] and three["S"] >= 2
    given, tg = sc.run("driver_phi_given")
    assert given["stages"] == 3 and [k for k, _ in _runs(tg)] == ["rc", "seeds", "rc"]
    for out in (one, three, given):
        assert np.array_equal(out["SEG"], sr.label(out["PHI"])) and out["surf"].shape == (3, out["S"])
    # stage j draws from seed + j*2^32: the second seeding of a run is not a replay of the first
    assert not np.array_equal(three["PHI"][:, :, 0], three["PHI"][:, :, -1])


def _runs(trace):
    out = []
    for r in trace:
        if not out or out[-1][1] != r["stage"]:
            out.append((r["kind"], r["stage"]))
    return out
