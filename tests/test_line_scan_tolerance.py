"""CPU: the tolerance budget of PDEIP_MODE_LINE_SCAN, from the reference's side only.

A scan evaluates a line's recurrences in another association order, so its solution differs from the serial one by a few units
in the last place.  Two things make the bounds of tests/test_gpu_line_scan.py meaningful for that:
  * the scan itself, in numpy float32 against the serial float32 Thomas solve: at most 4 ulp of the line's largest |x|;
  * the reference's own response to such differences: for every case of the GPU list the oracle, run one iteration at a time with
    every iterate plane moved by +-32 ulp after each iteration, stays within ONE TENTH of the bound the GPU test holds that case to.
A case that does not would leave both lists (line_scan_cases.CASES); none of them does.
"""
import numpy as np
import pytest

import line_scan_cases as lsc


@pytest.mark.parametrize("n", [2, 3, 9, 1025, 3840])
@pytest.mark.parametrize("data_term", [False, True])
def test_scan_thomas_is_within_4_ulp_of_the_serial_one(n, data_term):
    worst = 0.0
    for seed in range(4):
        rng = np.random.default_rng([n, seed, int(data_term)])
        f = np.float32
        before, after = rng.uniform(0.5, 5, n).astype(f), rng.uniform(0.5, 5, n).astype(f)
        off = (rng.uniform(0.5, 5, n) + rng.uniform(0.5, 5, n)).astype(f)  # the two off-line weights
        before[0], after[-1] = 0, 0
        b = (before + after + off).astype(f)
        d = (off * rng.uniform(-1, 1, n)).astype(f)
        if data_term:
            b = (b + rng.uniform(0.05, 2.3, n)).astype(f)
            d = (d + rng.uniform(-1.5, 1.5, n)).astype(f)
        a, c = (-before).astype(f), (-after).astype(f)
        serial, scan = lsc.thomas_serial(a, b, c, d), lsc.thomas_scan(a, b, c, d)
        ulp = float(np.spacing(np.max(np.abs(serial)).astype(f)))
        worst = max(worst, float(np.max(np.abs(scan.astype(np.float64) - serial.astype(np.float64)))) / ulp)
    print("n=%d data_term=%s: scan vs serial %.2f ulp of max|x|" % (n, data_term, worst))
    assert worst <= 4.0


def _check(oracle, c):
    rms_bound, max_bound = lsc.bounds(c)
    for it in c.iters:
        clean, noisy = lsc.disturbed_reference(oracle, c, it)
        for k, (rms, mx) in enumerate(lsc.differences(noisy, clean)):
            print("%s it=%d plane %d: +-%d ulp -> rms %.3g max %.3g" % (lsc.case_id(c), it, k, lsc.NOISE_ULP, rms, mx))
            assert rms <= rms_bound / 10, (lsc.case_id(c), it, k, rms)
            assert max_bound is None or mx <= max_bound / 10, (lsc.case_id(c), it, k, mx)


def _chunks(seq, n):
    return [seq[k::n] for k in range(n)]


@pytest.mark.parametrize("part", range(8))
def test_disturbed_reference_stays_within_a_tenth_of_the_bounds(oracle, part):
    for c in _chunks(lsc.CASES, 8)[part]:
        _check(oracle, c)


def test_disturbed_reference_at_c1_size(oracle):
    _check(oracle, lsc.C1_CASE)


def test_the_case_list_reaches_every_seam():
    """Both line directions at every boundary of the scan tree -1 / 0 / +1, every model, both kernel arities, G = 1, 2, 3."""
    lengths = {(c.model, n) for c in lsc.CASES for n in (c.nrows, c.ncols)}
    for b in (lsc.SCAN_VEC, lsc.SCAN_ROW * lsc.SCAN_VEC, lsc.SCAN_LANES * lsc.SCAN_VEC, lsc.SCAN_THREADS // 2 * lsc.SCAN_VEC, lsc.SCAN_THREADS * lsc.SCAN_VEC):
        for d in (-1, 0, 1):
            if b + d >= 3:
                assert ("elin4", b + d) in lengths and ("disp4", b + d) in lengths and ("pde4", b + d) in lengths, b + d
    for model in ("elin4", "pde4"):
        assert {lsc.scan_groups(model, n) for m, n in lengths if m == model} == {1, 2, 3}, model
    assert {c.model for c in lsc.CASES} == set(lsc.MODELS)
    assert all(lsc.scan_runs(c.model, c.nrows, c.ncols) for c in lsc.CASES + [lsc.C1_CASE])
    assert not lsc.scan_runs("elin4", 5300, 6) and not lsc.scan_runs("pde4", 10300, 5) and lsc.scan_runs("pde4", 5300, 6)
