"""CPU: the restatement of region competition (segmentation_ref.py) -- why the data term has a definition of its own, what the
strategies and the level do on the fixtures of segmentation_cases.py, and the decision margins of every end-to-end case against
the drift a single-ulp disturbance of DATA causes.  tests/test_gpu_segmentation.py compares the library with this restatement."""
import numpy as np
import pytest

import segmentation_cases as sc
import segmentation_ref as sr

F32 = np.float32


# ---- the data term ------------------------------------------------------------------------------------------------------------
def test_inverse_likelihood_equals_c_minus_p_away_from_zero():
    rng = np.random.default_rng(1)
    t = np.exp(rng.uniform(np.log(1e-3), np.log(40.0), 20000))
    cov = 1.7
    dist = (t * 2 * cov).astype(F32).reshape(100, 200, 1)
    r = sr.data_term(dist, np.ones_like(dist), np.ones_like(dist), [cov], sr.INVERSE)
    m = sr.data_term(dist, np.ones_like(dist), np.ones_like(dist), [cov], sr.INVERSE, form="matlab")
    assert (r["t"] > 1e-3 * 0.99).all()
    rel = np.abs(r["Q"] - m["Q"]) / r["Q"]
    print("Q against c - P where t > 1e-3: largest relative difference %.3g" % rel.max())
    assert rel.max() <= 1e-12


def test_the_m_form_jumps_where_dist_vanishes_and_q_does_not():
    """t < 1e-15: c - P is a multiple of c*2^-53, the size of the eps it is added to, so DATA steps by log(1 + c*2^-53/eps) ~ 0.17
    between neighbouring values of dist; Q = -c*expm1(-t) follows t."""
    cov = 1.0
    dist = np.linspace(0.0, 1.9e-15, 400).astype(F32).reshape(20, 20, 1)
    one = np.ones_like(dist)
    new = sr.data_term(dist, one, one, [cov], sr.INVERSE)
    old = sr.data_term(dist, one, one, [cov], sr.INVERSE, form="matlab")
    assert (new["t"] < 1e-15).all()
    step_new = np.abs(np.diff(new["DATA"].ravel().astype(np.float64))).max()
    step_old = np.abs(np.diff(old["DATA"].ravel().astype(np.float64))).max()
    print("largest step of DATA between neighbouring dist: the .m's form %.3g, Q %.3g; distinct values %d / %d"
          % (step_old, step_new, np.unique(old["DATA"]).size, np.unique(new["DATA"]).size))
    assert step_old > 0.1 and np.unique(old["DATA"]).size <= 10
    assert step_new < 0.02 and np.unique(new["DATA"]).size > 100
    c = new["c"][0]
    assert np.allclose(new["Q"].ravel(), c * new["t"].ravel(), rtol=1e-14, atol=0)


# ---- the strategies -----------------------------------------------------------------------------------------------------------
def test_strategies_differ_on_the_fixture():
    PHI, dist, DH = sc.stage_case((48, 64), 3)
    cov, _ = sr.variance(PHI, dist, 1.0)
    out = {k: sr.data_term(dist, PHI, DH, cov, v)["DATA"] for k, v in sr.STRATEGY.items()}
    for a, b in (("surface", "greedy"), ("surface", "inverse"), ("greedy", "inverse")):
        differ = np.mean(out[a].view(np.uint32) != out[b].view(np.uint32))
        print("%s vs %s: %.1f %% of DATA differ" % (a, b, 100 * differ))
        assert differ > 0.01


def test_one_segment_has_no_competitor():
    PHI, dist, DH = sc.stage_case((37, 53), 1)
    cov, _ = sr.variance(PHI, dist, 1.0)
    inv = sr.data_term(dist, PHI, DH, cov, sr.INVERSE)
    assert np.array_equal(inv["WC"], inv["Q"])
    for strat in (sr.SURFACE, sr.GREEDY):
        assert (sr.data_term(dist, PHI, DH, cov, strat)["WC"] == 0).all()


def test_max_ignores_nan_as_matlab_does():
    a, b, n = np.array([1.0]), np.array([2.0]), np.array([np.nan])
    assert sr.nanmax([n, a, b])[0] == 2 and sr.nanmax([a, n])[0] == 1 and np.isnan(sr.nanmax([n, n])[0])


def test_restatement_against_its_longdouble_recomputation():
    """The share of DATA that lands on the adjacent float when the same formulas run in np.longdouble stays under the cap of the
    GPU test (1 in 1 000): the cap leaves room for the last-bit differences of exp / expm1 / log and for nothing else."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("np.longdouble is no wider than float64 on this platform")
    worst = 0.0
    for shape in sc.STAGE_SHAPES:
        for S in sc.STAGE_S:
            PHI, dist, DH = sc.stage_case(shape, S)
            cov, _ = sr.variance(PHI, dist, 1.0)
            for strat in sr.STRATEGY.values():
                d64 = sr.data_term(dist, PHI, DH, cov, strat)["DATA"]
                dld = sr.data_term(dist, PHI, DH, cov, strat, ft=np.longdouble)["DATA"]
                ok = np.isfinite(d64) & np.isfinite(dld)
                assert np.array_equal(np.isnan(d64), np.isnan(dld))
                differ = d64[ok] != dld[ok]
                adjacent = np.nextafter(d64[ok], dld[ok]) == dld[ok]
                assert adjacent[differ].all()
                worst = max(worst, differ.mean())
    print("largest share of adjacent (not equal) DATA, float64 against longdouble: %.3g" % worst)
    assert worst <= 1e-3


# ---- the level ------------------------------------------------------------------------------------------------------------------
def test_small_segment_goes_at_iteration_one():
    out, trace = sc.run("dense48x64")
    assert trace[0]["sizes"][2] == 5 and trace[0]["removed"] == [2]
    assert trace[1]["sizes"].size == 3


def test_removal_on_an_even_iteration_recomputes_from_zero_models():
    """The fourth segment drops under the threshold at an even iteration: the terms are formed although the iteration is even, and
    from zero models -- a fresh call on the planes of the iteration before, whose models start at zero, gives the same bits."""
    D, PHI, _, args = sc.dense48x64()
    out, trace = sc.run("dense48x64")
    even = [r for r in trace if r["removed"] and r["iter"] % 2 == 0]
    assert len(even) == 1 and even[0]["recomputed"]
    it = even[0]["iter"]
    quiet = [r for r in trace if not r["removed"] and r["iter"] % 2 == 0]
    assert quiet and not any(r["recomputed"] for r in quiet)
    before = trace[it - 2]
    a = dict(args, iterations=1)
    fresh = sr.level(before["PHI"], D, fit_counter=before["fit_counter"], **a)
    assert np.array_equal(fresh["PHI"].view(np.uint32), trace[it - 1]["PHI"].view(np.uint32))
    assert np.array_equal(fresh["surf"].view(np.uint32), trace[it - 1]["surf"].view(np.uint32))
    assert out["kept"] == [0, 1] and out["S"] == 2


def test_level_finds_the_two_planes():
    D, PHI, truth, args = sc.dense48x64()
    out, _ = sc.run("dense48x64")
    lab = sr.label(out["PHI"])
    got = np.zeros_like(lab)
    for i, k in enumerate(out["kept"]):
        got[lab == i + 1] = k + 1
    planes = truth > 0
    share = np.mean(got[planes] == truth[planes])
    print("pixels of the two planes labelled as the ground truth: %.2f %%" % (100 * share))
    assert share >= 0.95


def test_no_segment_left():
    D, PHI, _, args = sc.dense48x64()
    out = sr.level(PHI, D, **dict(args, srem_thr=0.9))
    assert out["S"] == 0 and out["kept"] == [] and out["PHI"].shape[2] == 0


def test_label():
    PHI = np.full((3, 4, 3), -1, F32)
    PHI[0, 0, 0] = 1
    PHI[1, 1, 2] = 1
    PHI[2, 2, 0] = PHI[2, 2, 1] = 1
    PHI[0, 1, 1] = 0  # PHI > 0: a zero is outside
    PHI[0, 2, 1] = np.nan
    lab = sr.label(PHI)
    want = np.zeros((3, 4), np.int32)
    want[0, 0], want[1, 1] = 1, 3
    assert np.array_equal(lab, want)


# ---- decision margins against the drift -------------------------------------------------------------------------------------------
def measured_drift(name):
    (out, trace), (pout, ptrace) = sc.run(name), sc.run(name, perturbed=True)
    assert len(trace) == len(ptrace) and out["kept"] == pout["kept"]
    drift = 0.0
    for a, b in zip(trace, ptrace):
        assert a["removed"] == b["removed"] and np.array_equal(a["sizes"], b["sizes"])
        assert np.array_equal(sr.mask(a["PHI"]), sr.mask(b["PHI"])), "%s: a mask changed at iteration %d" % (name, a["iter"])
        assert np.array_equal(a["surf"].view(np.uint32), b["surf"].view(np.uint32)), "%s: a surface changed" % name
        drift = max(drift, float(np.max(np.abs(a["PHI"].astype(np.float64) - b["PHI"]))))
    return drift


@pytest.mark.parametrize("name", list(sc.END_TO_END))
def test_drift_and_decision_margins(name):
    drift = measured_drift(name)
    out, trace = sc.run(name)
    min_phi = min(min(r["min_phi"] for r in trace), float(np.min(np.abs(out["PHI"]))))
    min_size = min(r["min_size"] for r in trace)
    min_ransac = min(r["min_ransac"] for r in trace)
    rec = sc.DRIFT[name]
    print("%s: drift %.3g (recorded %.3g); smallest |PHI| at a decision %.3g, size to threshold %.3g, RANSAC sum margin %.3g"
          % (name, drift, rec, min_phi, min_size, min_ransac))
    assert drift <= rec, "DRIFT[%r] = %g is smaller than the measured %g" % (name, rec, drift)
    assert rec <= 2 * drift + 1e-12, "DRIFT[%r] = %g is not the measured value (%g)" % (name, rec, drift)
    assert min_phi > 10 * rec and min_size > 10 * rec and min_ransac > 10 * rec
