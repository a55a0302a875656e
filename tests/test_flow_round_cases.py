"""CPU: the cases of tests/flow_round_cases.py reach what they claim.  The loop bounds of k_crosscheck_final, k_flow_err_final,
k_flow_maxmag, k_splat_clear and k_inpaint_merge are restated here in plain Python from the table of constants, and the shapes are
shown to run each loop the stated number of times.  These are conditions on the inputs: if an edit to a case breaks one, this file
fails, not the GPU test."""
import math

import numpy as np
import pytest

import crosscheck_ref as cr
import flow_round_cases as fc

F32, F64 = np.float32, np.float64


def test_the_constants_are_those_of_the_kernels():
    """Read from the sources, so that a changed constant fails here and the cases are rebuilt around it."""
    import os
    import re

    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pde-based-image-processing_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in ("pdeip_crosscheck.hpp", "pdeip_flowviz.hpp", "pdeip_interp.hpp", "pdeip_inpaint.hpp",
                                                             "pdeip_interp.hip", "pdeip_inpaint.hip")}
    const = lambda f, name: int(re.search(r"constexpr int %s = (\d+);" % name, text[f]).group(1))
    assert const("pdeip_crosscheck.hpp", "BLOCK") == const("pdeip_flowviz.hpp", "BLOCK") == const("pdeip_interp.hpp", "BLOCK") == fc.BLOCK
    assert const("pdeip_inpaint.hpp", "FLAT_BLOCK") == fc.BLOCK
    assert const("pdeip_crosscheck.hpp", "FINAL_BLOCK") == fc.FINAL_BLOCK and const("pdeip_crosscheck.hpp", "FINAL_BATCH") == fc.FINAL_BATCH
    assert const("pdeip_flowviz.hpp", "ERR_PER_THREAD") * fc.BLOCK == fc.ERR_TILE and const("pdeip_flowviz.hpp", "MAXMAG_BLOCKS") == fc.MAXMAG_BLOCKS
    for f in ("pdeip_interp.hip", "pdeip_inpaint.hip"):
        assert "if (blocks > 256 * 16) blocks = 256 * 16;" in text[f] and fc.FLAT_BLOCKS == 256 * 16
    assert all(len(v) == 2 and isinstance(v[1], str) for v in fc.CONSTANTS.values())


# ---- k_crosscheck_final ----------------------------------------------------------------------------------------------------------
# nparts: (batched, tail) iterations of thread 0, of thread 1023
ITERATIONS = {
    1024: ((0, 1), (0, 1)),
    1025: ((0, 2), (0, 1)),
    3072: ((0, 3), (0, 3)),
    3073: ((1, 0), (0, 3)),
    3074: ((1, 0), (0, 3)),
    4096: ((1, 0), (1, 0)),
    4097: ((1, 1), (1, 0)),
    4098: ((1, 1), (1, 0)),
    7168: ((1, 3), (1, 3)),
    7169: ((2, 0), (1, 3)),
    8193: ((2, 1), (2, 0)),
}
PATTERNS = {
    "tail only": lambda b, t: b == 0 and t >= 1,
    "batch only": lambda b, t: b == 1 and t == 0,
    "batch then tail": lambda b, t: b >= 1 and t >= 1,
    "two batches": lambda b, t: b == 2,
    "a batch followed by three tails": lambda b, t: b == 1 and t == 3,
}


def test_final_iterations_of_every_shape():
    seen = set()
    for what in ("disp", "flow"):
        for shape in fc.shapes_of(what):
            nparts = fc.nparts_of(shape)
            seen.add(nparts)
            assert (fc.final_iterations(nparts, 0), fc.final_iterations(nparts, 1023)) == ITERATIONS[nparts], shape
            for t in (0, 1, 2, 1022, 1023):   # whatever the split, a thread folds each of its parts once
                b, tail = fc.final_iterations(nparts, t)
                assert fc.FINAL_BATCH * b + tail == len(range(t, nparts, fc.FINAL_BLOCK))
    assert seen == set(ITERATIONS)
    assert fc.shapes_of("disp") == fc.CROSS_SHAPES and all(s[0] >= 2 for s in fc.shapes_of("flow")) and len(fc.shapes_of("flow")) == 11
    # the largest plane of the suite before these cases, 270 x 480, left one part per thread at the most
    assert fc.nparts_of((270, 480)) == 960 and fc.final_iterations(960, 0) == (0, 1) and fc.final_iterations(960, 1023) == (0, 0)


@pytest.mark.parametrize("thread", (0, 1023))
@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_the_list_holds_every_pattern_for_the_first_and_the_last_thread(pattern, thread):
    for what in ("disp", "flow"):
        hits = [s for s in fc.shapes_of(what) if PATTERNS[pattern](*fc.final_iterations(fc.nparts_of(s), thread))]
        assert hits, "%s: no %s shape gives thread %d '%s'" % (pattern, what, thread, pattern)


def test_tall_shapes():
    (a, b) = fc.TALL_SHAPES
    assert fc.nparts_of(a) == 2 * 1537 == 3074 and fc.nparts_of(b) == 3 * 1366 == 4098
    for what in ("disp", "flow"):
        ref, tree, mag = fc.cross_want(what, a, "integers")
        assert a[0] - fc.BLOCK == 1   # every second part holds one live row: at most one defined pixel
        import reduce_tree_ref as rt

        k, d, s, m = rt.crosscheck_thread_values(ref["kept_mask"], ref["defined_mask"], mag, *a)
        per_part = d.sum(axis=1)
        assert per_part[1::2].max() == 1 and per_part[0::2].min() >= 250 and not d[1::2, 1:].any()


# ---- the residual is the gathered plane itself -----------------------------------------------------------------------------------
@pytest.mark.parametrize("family", fc.FAMILIES)
def test_residuals_are_the_gathered_planes(family):
    for shape in ((1, 1025), (2, 4097), (257, 1537)):
        D0, D1, tol = fc.disp_case(shape, family)
        ref = cr.disp_crosscheck(D0, D1, tol)
        d = ref["defined_mask"]
        assert np.array_equal(ref["r"][d], D1.astype(F64)[d]) and not d[np.isnan(D1)].any()
        if shape[0] < 2:
            continue
        Uf, Vf, Ub, Vb, (a, b) = fc.flow_case(shape, family)
        ref = cr.flow_crosscheck(Uf, Vf, Ub, Vb, a, b)
        d = ref["defined_mask"]
        with np.errstate(invalid="ignore"):
            want = np.sqrt(Ub.astype(F64) ** 2 + Vb.astype(F64) ** 2)
        assert np.array_equal(ref["err64"][d], want[d]) and not d[np.isnan(Ub)].any()
        if family == "binades":
            assert np.array_equal(ref["err64"][d], np.abs(Ub.astype(F64))[d])
            m, e = np.frexp(ref["err64"][d])
            assert e.min() == -19 and e.max() == 21 and len(np.unique(e)) == 41   # m 2^e with m in [1, 2): frexp's exponent is e + 1


@pytest.mark.parametrize("what", ("disp", "flow"))
def test_largest_value_sweep(what):
    assert fc.nparts_of(fc.SWEEP_SHAPE) == 7169
    rounds = set()
    for part in fc.SWEEP_PARTS:
        ref, tree, mag = fc.cross_want(what, fc.SWEEP_SHAPE, "integers", fc.sweep_pixel(part))
        assert ref["defined"] == mag.size and ref["max"] == tree["max"] == fc.SWEEP_VALUE
        at = np.argwhere(mag == fc.SWEEP_VALUE)
        assert len(at) == 1 and at[0][1] == part and np.sort(mag.ravel())[-2] <= 13
        rounds.add((part % fc.FINAL_BLOCK, part // fc.FINAL_BLOCK))
    # (final thread, its round): thread 0 runs two batches (rounds 0..3, 4..7), thread 1023 one and three tail steps (rounds 4..6) --
    # the first step of each batch, a step inside, the last; the first and the last tail step
    assert rounds == {(0, 0), (1023, 0), (0, 1), (1023, 2), (0, 3), (1023, 3), (0, 4), (1023, 4), (1023, 6), (0, 7)}
    assert fc.final_iterations(7169, 0) == (2, 0) and fc.final_iterations(7169, 1023) == (1, 3)


# ---- the flow errors -------------------------------------------------------------------------------------------------------------
def test_error_sizes_and_cases():
    assert [fc.err_tiles(n) for n in fc.ERR_SIZES] == [256, 257, 512, 513]
    assert [math.ceil(fc.err_tiles(n) / fc.BLOCK) for n in fc.ERR_SIZES] == [1, 2, 2, 3], "rounds of k_flow_err_final"
    assert fc.err_tiles(270 * 480) == 64
    cases = fc.error_cases()
    assert len(cases) == len(set(cases)) == 21
    acos0 = math.degrees(math.acos(0.0))
    for case in cases:
        ref, tree = fc.error_want(case)
        n, family, masked, peak, dead = case
        assert ref["counted"].shape == (n, 1) and 0 < ref["count"] and (ref["count"] < n) == (masked or dead is not None or family == "binades")
        if family == "integers":
            ang = ref["ang_plane64"][ref["counted"]]
            assert set(np.unique(ang)) == {0.0, np.arccos(0.0) * 57.29577951308232} and abs(acos0 - 90.0) < 1e-13
        if peak is not None:
            at = np.flatnonzero(ref["epe_plane64"].ravel() == 2.0 + fc.ERR_PEAK_A ** 2)
            assert len(at) == 1 and at[0] // fc.ERR_TILE == peak and ref["max_epe"] == 902.0
            assert np.sort(ref["epe_plane64"].ravel())[-2] == 18.0
        if dead is not None:
            import reduce_tree_ref as rt

            parts = rt.flow_error_partials(ref["counted"].ravel(), ref["epe_plane64"].ravel(), ref["ang_plane64"].ravel())
            assert all(not p[dead:].any() for p in parts[:3]) and np.all(parts[3][dead:] == -1.0) and np.all(parts[0][:dead] > 2000)


# ---- the automatic maximum -------------------------------------------------------------------------------------------------------
def maxmag_reader(n, vec, pos):
    """(thread, stride round, 'vec' or 'tail') of the load of k_flow_maxmag that reads pixel pos: grid min(ceil(n / 256), 1024)."""
    threads = min(-(-n // fc.BLOCK), fc.MAXMAG_BLOCKS) * fc.BLOCK
    done = (n >> 2) << 2 if vec else 0
    if pos < done:
        return (pos >> 2) % threads, (pos >> 2) // threads, "vec"
    return (pos - done) % threads, (pos - done) // threads, "tail"


def test_maxmag_positions():
    S = fc.ONE_STRIDE
    assert S == 262144 and sorted(fc.MAXMAG_SCALAR) == [S, S + 1, 2 * S + 1] and sorted(fc.MAXMAG_VEC) == [4 * S, 4 * S + 3, 4 * S + 4, 4 * S + 7]
    assert maxmag_reader(270 * 480, False, 270 * 480 - 1)[1] == 0 and maxmag_reader(270 * 480, True, 270 * 480 - 1)[1] == 0
    got = {n: [maxmag_reader(n, False, p) for p in fc.maxmag_positions(fc.MAXMAG_SCALAR, n)] for n in fc.MAXMAG_SCALAR}
    assert got[S] == [(0, 0, "tail"), (S - 1, 0, "tail")]
    assert got[S + 1] == [(0, 0, "tail"), (S - 1, 0, "tail"), (0, 1, "tail")]
    assert got[2 * S + 1] == [(0, 0, "tail"), (S - 1, 0, "tail"), (0, 1, "tail"), (0, 2, "tail")]
    got = {n: [maxmag_reader(n, True, p) for p in fc.maxmag_positions(fc.MAXMAG_VEC, n)] for n in fc.MAXMAG_VEC}
    assert got[4 * S] == [(S - 1, 0, "vec")]
    assert got[4 * S + 3] == [(S - 1, 0, "vec"), (0, 0, "tail"), (2, 0, "tail")]
    assert got[4 * S + 4] == [(S - 1, 0, "vec"), (0, 1, "vec"), (0, 1, "vec")]
    assert got[4 * S + 7] == [(S - 1, 0, "vec"), (0, 1, "vec"), (0, 0, "tail"), (2, 0, "tail")]
    assert math.hypot(*fc.PEAK) == 5.0


# ---- the flat sweeps -------------------------------------------------------------------------------------------------------------
def test_flat_sweeps():
    assert fc.ONE_SWEEP == 1048576
    assert [a * b for a, b in fc.SPLAT_SHAPES] == [fc.ONE_SWEEP, 1049600] and [a * b for a, b in fc.MERGE_SHAPES] == [fc.ONE_SWEEP, 1049600, fc.ONE_SWEEP + 1]
    assert 270 * 480 < fc.ONE_SWEEP   # the largest plane of the suite before these cases
    # the closed form the GPU test uses on the large planes, against the restatement on a small one: zero flow, two channels
    import interp_ref as ir

    rng = np.random.default_rng(5)
    I0, I1 = (np.asfortranarray(rng.random((37, 53, 2), dtype=F32)) for _ in range(2))
    zero = np.zeros((37, 53), F32, order="F")
    Ut, Vt, cost = ir.flow_splat(zero, zero, 0.5, I0, I1)[:3]
    want = (np.abs(I0[:, :, 0].astype(F64) - I1[:, :, 0].astype(F64)) + np.abs(I0[:, :, 1].astype(F64) - I1[:, :, 1].astype(F64))).astype(F32)
    assert not Ut.view(np.uint32).any() and not Vt.view(np.uint32).any() and np.array_equal(cost, want)
    nan = np.full((37, 53), np.nan, F32, order="F")
    assert all(np.isnan(p).all() for p in ir.flow_splat(nan, nan, 0.5, I0, I1)[:3])
