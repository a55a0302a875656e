"""CPU: the restatement of the sparse driver (sparse_ref.py) and its fixtures (sparse_cases.py).  Ties nanmedfilt2 to an independent
statement (numpy's nanmedian over zero-padded windows), the restatement's generateSeeds() / driver to the pinned seeds_ref, and
proves -- as test_seeds_ref.py does for the dense fixtures -- that no sparse fixture decides anything on a knife's edge: with DRIFT the
measured change of PHI under a one-ulp perturbation of DATA, every `>= 0` / `> 0` decision on PHI and every `AA > 0.05` decision
clears DRIFT tenfold, every count differs from 20 by at least 3 pixels, the largest component beats the second by at least 3 pixels,
and every RANSAC `sum < best` comparison has a relative margin of at least 1e-3."""
import functools
import warnings

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

import seeds_cases as sc
import seeds_ref as gs
import segmentation_ref as sr
import sparse_cases as spc
import sparse_ref as sp
from test_seeds_ref import _decisions, _iters, _runs, margins

F32 = np.float32


def _same_bits(got, want, what):
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: NaN pattern differs" % what
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok], want[ok]), "%s: values differ" % what  # by value: which zero is not part of the contract


def _nanmedian_windows(A):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # all-NaN slices, Inf - Inf
        return np.nanmedian(sliding_window_view(np.pad(A.astype(np.float64), 1), (3, 3)), axis=(2, 3)).astype(F32)


# ---- 1. nanmedfilt2 against an independent statement ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", spc.FILTER_NAMES)
def test_nanmedfilt2_equals_nanmedian_of_padded_windows(name):
    A = spc.filter_cases()[name]
    _same_bits(sp.nanmedfilt2(A), _nanmedian_windows(A), name)


def test_nanmedfilt2_equals_nanmedian_on_random_planes():
    for shape in spc.RANDOM_SHAPES:
        for share in spc.NAN_SHARES:
            A = spc.random_plane(shape, share)
            planes = A[:, :, None] if A.ndim == 2 else A
            got = sp.nanmedfilt2(A)
            got = got[:, :, None] if got.ndim == 2 else got
            for f in range(planes.shape[2]):
                _same_bits(got[:, :, f], _nanmedian_windows(planes[:, :, f]), "%s at %g, frame %d" % (shape, share, f))


# ---- 2. the filter cases hold what they claim ---------------------------------------------------------------------------------------
def _window_nans(A, i, j):
    n = 0
    for di, dj in spc.WINDOW:
        if 0 <= i + di < A.shape[0] and 0 <= j + dj < A.shape[1]:
            n += int(np.isnan(A[i + di, j + dj]))
    return n


def test_filter_cases_hold_what_they_claim():
    cases = spc.filter_cases()
    assert sorted(cases) == spc.FILTER_NAMES
    A = cases["nan_counts_interior"]
    assert [_window_nans(A, 2, 5 * c + 2) for c in range(10)] == list(range(10))
    out = sp.nanmedfilt2(A)
    assert np.isnan(out[2, 47]) and not np.isnan(out[2, 42])  # nine NaNs: NaN; eight: the one number
    A = cases["nan_counts_edge"]
    assert [_window_nans(A, 0, 5 * c + 2) for c in range(7)] == list(range(7))
    out = sp.nanmedfilt2(A)
    assert out[0, 32] == 0 and out[0, 27] == 0  # six NaNs: the three zeros alone; five: three zeros and one number, whose middle two are zeros
    for c in range(5):
        A = cases["corner_nan%d" % c]
        assert _window_nans(A, 0, 0) == c and (A[~np.isnan(A)] > 0).all()
        assert sp.nanmedfilt2(A)[0, 0] == 0  # five zeros among at most nine numbers, all others positive: the median is a zero
    # every even count with two distinct middle values whose float32 mean is inexact
    A = cases["even_inexact"]
    out = sp.nanmedfilt2(A)
    for e, n in enumerate((2, 4, 6, 8)):
        w = np.sort(np.array([A[2 + di, 5 * e + 2 + dj] for di, dj in spc.WINDOW]))
        assert (~np.isnan(w)).sum() == n
        a, b = w[n // 2 - 1], w[n // 2]
        assert a != b and b == np.nextafter(a, F32(np.inf))
        exact = (np.float64(a) + np.float64(b)) * 0.5
        assert np.float64(F32(exact)) != exact  # the mean is no float32
        assert out[2, 5 * e + 2] == F32(exact) and out[2, 5 * e + 2] in (a, b)
    A = cases["inf_pairs"]
    out = sp.nanmedfilt2(A)
    assert np.isnan(out[2, 2]) and out[2, 7] == np.inf and out[2, 12] == -np.inf and np.isnan(out[2, 17])
    assert (sp.nanmedfilt2(cases["plateau_constant"])[1:-1, 1:-1] == 7).all()
    T = cases["plateau_ties"]
    assert len(np.unique(T)) == 3
    Z = cases["both_zeros"]
    assert (np.signbit(Z) & (Z == 0)).any() and (~np.signbit(Z) & (Z == 0)).any() and np.isnan(Z).any()
    N = sp.nanmedfilt2(cases["all_nan"])
    assert np.isnan(N[1:-1, 1:-1]).all() and (N[0] == 0).all() and (N[-1] == 0).all() and (N[:, 0] == 0).all() and (N[:, -1] == 0).all()


# ---- 3. with the plain builder, gamma0 = 0.01 and the dense constants the restatement is seeds_ref's ------------------------------
def test_dense_form_reproduces_seeds_ref():
    want, wtrace = sc.run("planes60x80_o1")
    a = sc.SEEDS_CASES["planes60x80_o1"]()
    trace = []
    got = sp.generate_seeds(a["D"], a["order"], a["sigmaLim"], a["cset_vect"], a["iterations"], AA=a["AA"], seeds=a["seeds"],
                            scl_factor=a["scl_factor"], pyr_scl=a["pyr_scl"], seed=a["seed"], prm=a["prm"], pyramid=sp.plain_pyramid,
                            gamma0=sp.GAMMA0_DENSE, defaults=gs.DENSE, trace=trace)
    assert got["S"] == want["S"] and got["fit_counter"] == want["fit_counter"] and got["gamma"] == want["gamma"]
    assert got["PHI"].tobytes() == want["PHI"].tobytes() and got["surf"].tobytes() == want["surf"].tobytes()
    assert _decisions(got, trace) == _decisions(want, wtrace)
    want, wtrace = sc.run("driver_seeds1")
    a = sc.DRIVER_CASES["driver_seeds1"]()
    trace = []
    got = sp.disp_segmentation_sparse(a.pop("Din"), trace=trace, pyramid=sp.plain_pyramid, gamma0=sp.GAMMA0_DENSE, seeds_defaults=gs.DENSE,
                                      seg_defaults=sr.DENSE, driver_defaults=gs.DRIVER, zero_nans=True, **a)
    assert got["S"] == want["S"] and got["stages"] == want["stages"]
    assert got["PHI"].tobytes() == want["PHI"].tobytes() and got["surf"].tobytes() == want["surf"].tobytes()
    assert np.array_equal(got["SEG"], want["SEG"]) and _decisions(got, trace) == _decisions(want, wtrace)


# ---- 4.-6. the driver fixtures ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def measured_drift(name):
    out, trace = spc.run(name)
    pout, ptrace = spc.run(name, perturbed=True)
    assert _decisions(out, trace) == _decisions(pout, ptrace), "%s: the perturbation changed a decision" % name
    drift = 0.0
    for a, b in zip(_iters(trace), _iters(ptrace)):
        drift = max(drift, float(np.max(np.abs(a["PHI"].astype(np.float64) - b["PHI"]))))
    if out["S"]:
        drift = max(drift, float(np.max(np.abs(out["PHI"].astype(np.float64) - pout["PHI"]))))
    return drift


@pytest.mark.parametrize("name", spc.ALL)
def test_drift_and_decision_margins(name):
    drift = measured_drift(name)
    out, trace = spc.run(name)
    m = margins(out, trace)
    rec = spc.DRIFT[name]
    print("%s: drift %.3g (recorded %.3g); margins %r" % (name, drift, rec, m))
    assert drift <= rec, "DRIFT[%r] = %g is smaller than the measured %g" % (name, rec, drift)
    assert rec <= 2 * drift + 1e-12, "DRIFT[%r] = %g is not the measured value (%g)" % (name, rec, drift)
    assert m["phi"] > 10 * rec and m["aa"] > 10 * rec
    assert m["count"] >= 3 and m["size"] >= 3
    assert m["component"] >= 3
    assert m["ransac"] >= 1e-3


def test_fixture_geometry():
    D = spc.sparse_map()
    assert D.shape == (60, 80) and np.isnan(D[26:33, 50:58]).all()
    share = float(np.isnan(D).mean())
    assert 0.13 < share < 0.19  # 15 % random NaNs plus the 7x8 block
    P = sp.sparse_pyramid(D, spc.SCL, spc.PYR)
    assert [p.shape for p in P] == [(60, 80), (45, 60), (34, 45)]
    for p in P:  # every scale keeps a NaN (the nan_fill and dist_cap paths run) and at most 10 %
        assert np.isnan(p).any() and float(np.isnan(p).mean()) <= 0.10
    for name in spc.ALL:
        out, _ = spc.run(name)
        if "Dp" in out:
            assert len(out["Dp"]) == 3 and all(np.array_equal(np.isnan(a), np.isnan(b)) for a, b in zip(out["Dp"], P))


def test_fixtures_are_what_they_claim():
    for name, ncoef in (("sp_seeds_o1", 3), ("sp_seeds_o2", 6)):
        out, trace = spc.run(name)
        assert out["sizes"] == [(60, 80), (45, 60), (34, 45)] and out["surf"].shape[0] == ncoef
        assert {r["visit"] for r in trace} == set(range(6)) and max(r["iter"] for r in _iters(trace)) == 8
        assert 1 <= out["S"] <= 3
    out, trace = spc.run("sp_tiny_aa")
    assert out["S"] == 0 and out["fit_counter"] == 0 and [r["count"] for r in trace] == [1, 1, 1]
    assert out["gamma"] == 0.005 * 0.8 * 0.8 * 0.8  # gamma shrinks from the sparse driver's start
    band, _ = spc.run("sp_band")
    assert band["S"] >= 1 and (band["PHI"][:, 31:43, :] < 0).all()
    a = spc.SEEDS_CASES["sp_short_cset"]()
    assert len(a["cset_vect"]) < a["iterations"] and a["cset_vect"] == sc.CSET_DRIVER[:3]
    _, trace = spc.run("sp_short_cset")
    assert min(r["min_ransac"] for r in _iters(trace)) < np.inf  # this fixture does compare sums
    rc, trace = spc.run("sp_rc")
    assert rc["S"] == 2 and {r["visit"] for r in trace} == set(range(6))


def test_driver_branches():
    one, t1 = spc.run("sp_driver_seeds1")
    assert one["stages"] == 1 and one["S"] == 1 and {r["kind"] for r in t1} == {"seeds"} and one["surf"].shape == (6, 1)  # polyorder 2 by default
    three, t3 = spc.run("sp_driver_seeds3")
    assert three["stages"] == 4 and [k for k, _ in _runs(t3)] == ["seeds", "rc", "seeds", "rc"] and three["S"] >= 2
    assert three["surf"].shape == (3, three["S"])
    given, tg = spc.run("sp_driver_phi_given")
    assert given["stages"] == 3 and [k for k, _ in _runs(tg)] == ["rc", "seeds", "rc"] and given["surf"].shape[0] == 6
    for out in (one, three, given):
        assert np.array_equal(out["SEG"], sr.label(out["PHI"]))


def test_the_sparse_pyramid_and_gamma_matter():
    """No test passes for the wrong reason: the plain pyramid (what drivers.generateSeeds(sparse=True) runs) and the dense gamma
    give different results on these fixtures."""
    name = "sp_seeds_o1"
    out, trace = spc.run(name)
    plain, ptrace = spc.run_variant(name, pyramid=sp.plain_pyramid)
    counts = [r["count"] for r in trace if "count" in r]
    pcounts = [r["count"] for r in ptrace if "count" in r]
    masks = [sr.mask(r["PHI"]).tobytes() for r in _iters(trace)]
    pmasks = [sr.mask(r["PHI"]).tobytes() for r in _iters(ptrace)]
    assert counts != pcounts or masks != pmasks
    dense_gamma, _ = spc.run_variant(name, gamma0=sp.GAMMA0_DENSE)
    assert dense_gamma["S"] != out["S"] or float(np.max(np.abs(dense_gamma["PHI"].astype(np.float64) - out["PHI"]))) > 40 * spc.DRIFT[name]
