"""CPU: tests/reduce_tree_ref.py is the documented order and no other.  On the `integers` cases of tests/flow_round_cases.py, where
every sum is exact, it equals the integer sums and math.fsum; on 2^53, 1, 1 placed in chosen lanes, waves, parts, pixels and tiles it
gives the bits the documented order implies by hand -- (2^53 + 1) + 1 = 2^53 where the large value comes first, 2^53 + (1 + 1) =
2^53 + 2 where the ones meet first -- and not those of the other order; threads that hold nothing change no bit; and every
`binades` case tells the documented order from math.fsum, from a single ascending chain, from the butterfly run backwards and, where
every final thread runs a batch of four, from the batch folded last part first (at 3073 and 3074 parts one or two threads do: there
the `hand` cases tell).  These are conditions on the restatement and on the cases: the GPU tests compare with them bit for bit."""
import math

import numpy as np
import pytest

import flow_round_cases as fc
import reduce_tree_ref as rt

F64 = np.float64
BIG = 2.0 ** 53
REVERSED = rt.STEPS[::-1]
CROSS = [(w, s) for w in ("disp", "flow") for s in fc.shapes_of(w)]
cross_id = lambda c: "%s-%dx%d" % (c[0], c[1][0], c[1][1])


# ---- exact sums ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,shape", CROSS, ids=[cross_id(c) for c in CROSS])
def test_integer_cross_cases_are_exact(what, shape):
    ref, tree, mag = fc.cross_want(what, shape, "integers")
    d = ref["defined_mask"]
    assert np.all(mag[d] == np.round(mag[d])) and mag[d].max() <= 13
    total = int(mag[d].astype(np.int64).sum())
    assert tree["kept"] == ref["kept"] == int(ref["kept_mask"].sum()) and tree["defined"] == ref["defined"] == int(d.sum())
    assert tree["sum"] == total and rt.bits(tree["mean"]) == rt.bits(F64(total) / F64(ref["defined"])) == rt.bits(ref["mean"])
    assert rt.bits(tree["max"]) == rt.bits(ref["max"]) and tree["nparts"] == fc.nparts_of(shape)
    assert 0 < ref["kept"] < ref["defined"] < shape[0] * shape[1]


@pytest.mark.parametrize("case", [c for c in fc.error_cases() if c[1] == "integers"], ids=fc.error_id)
def test_integer_error_cases_are_exact(case):
    ref, tree = fc.error_want(case)
    c = ref["counted"]
    epe = ref["epe_plane64"][c]
    assert np.all(epe == np.round(epe))
    total = int(epe.astype(np.int64).sum())
    assert tree["count"] == ref["count"] == int(c.sum()) and tree["sum_epe"] == total
    assert rt.bits(tree["mean_epe"]) == rt.bits(F64(total) / F64(ref["count"])) == rt.bits(ref["mean_epe"])
    assert rt.bits(tree["max_epe"]) == rt.bits(ref["max_epe"]) and tree["ntiles"] == fc.err_tiles(case[0])


# ---- 2^53, 1, 1 ------------------------------------------------------------------------------------------------------------------
def _lanes(**at):
    v = np.zeros(64)
    for lane, x in at.items():
        v[int(lane[1:])] = x
    return v


def test_wave_tree_order_by_hand():
    # lanes 0, 1, 3: the step d = 2 adds lane 3 to lane 1 first (1 + 1), d = 1 then adds that to lane 0
    v = _lanes(l0=BIG, l1=1.0, l3=1.0)
    assert rt.wave_tree(v) == BIG + 2.0 and rt.wave_tree(v, REVERSED) == BIG
    # lanes 0, 32, 33: d = 32 adds lane 32 to lane 0 (2^53 + 1 = 2^53) and lane 33 to lane 1, which d = 1 adds last; backwards,
    # d = 1 adds lane 33 to lane 32 first
    v = _lanes(l0=BIG, l32=1.0, l33=1.0)
    assert rt.wave_tree(v) == BIG and rt.wave_tree(v, REVERSED) == BIG + 2.0
    # lanes 0, 32, 16 meet the large value one at a time in either direction
    v = _lanes(l0=BIG, l32=1.0, l16=1.0)
    assert rt.wave_tree(v) == BIG and rt.wave_tree(v, REVERSED) == BIG
    # every lane ends with the same bits: the tree is the same seen from any lane
    rng = np.random.default_rng(3)
    w = np.ldexp(1.0 + rng.random(64), rng.integers(-20, 21, size=64))
    lane = np.arange(64)
    full = w.copy()
    for d in rt.STEPS:
        full = full + full[lane ^ d]
    assert np.all(full.view(np.uint64) == full.view(np.uint64)[0]) and rt.bits(full[0]) == rt.bits(rt.wave_tree(w))
    assert rt.wave_tree_max(_lanes(l5=3.0, l63=7.0) - 1.0) == 6.0 and rt.wave_tree_max(np.full(64, -1.0)) == -1.0


def test_workgroup_fold_order_by_hand():
    def waves(**at):
        v = np.zeros(256)
        for w, x in at.items():
            v[64 * int(w[1:]) + 9] = x
        return v

    assert rt.workgroup_fold(waves(w0=BIG, w1=1.0, w2=1.0)) == BIG        # (2^53 + 1) + 1
    assert rt.workgroup_fold(waves(w0=1.0, w1=1.0, w3=BIG)) == BIG + 2.0   # (1 + 1) + 0 + 2^53
    assert rt.workgroup_fold(waves(w0=BIG, w2=1.0, w3=1.0)) == BIG
    assert rt.workgroup_fold(np.full(256, -1.0), True) == -1.0


def _parts(n, **at):
    p = np.zeros(n)
    for k, x in at.items():
        p[int(k[1:])] = x
    return p


def test_final_fold_order_by_hand():
    # one final thread: parts t, t + 1024, t + 2048 in ascending order
    assert rt.final_fold(_parts(3000, p5=BIG, p1029=1.0, p2053=1.0)) == BIG
    assert rt.final_fold(_parts(3000, p5=1.0, p1029=1.0, p2053=BIG)) == BIG + 2.0
    # three final threads of one wave: the butterfly, where a single chain over the parts gives the other bits
    p = _parts(3000, p0=BIG, p1=1.0, p3=1.0)
    assert rt.final_fold(p) == BIG + 2.0 and rt.final_fold(p, final="chain") == BIG
    # three waves of the final workgroup: ascending
    assert rt.final_fold(_parts(1024, p0=BIG, p64=1.0, p960=1.0)) == BIG
    assert rt.final_fold(_parts(1024, p0=1.0, p64=1.0, p960=BIG)) == BIG + 2.0
    # the fifth round of a thread (beyond one batch of four) still comes after the fourth
    assert rt.final_fold(_parts(5000, p7=BIG, p3079=1.0, p4103=1.0)) == BIG
    assert rt.final_fold(_parts(5000, p7=1.0, p3079=1.0, p4103=BIG)) == BIG + 2.0
    assert rt.final_fold(_parts(5000, p4999=6.0) - 1.0, True) == 5.0
    # the wrong order that folds a batch last part first: thread 7 of 5000 parts runs one batch (7 < 5000 - 3072), thread 1000 of 4000 parts none
    p = _parts(5000, p7=BIG, p1031=1.0, p2055=1.0)
    assert rt.final_fold(p) == BIG and rt.final_fold(p, final="batch_descending") == BIG + 2.0
    p = _parts(4000, p1000=BIG, p2024=1.0, p3048=1.0)
    assert rt.final_fold(p) == BIG and rt.final_fold(p, final="batch_descending") == BIG
    rng = np.random.default_rng(9)
    p = np.ldexp(1.0 + rng.random(3000), rng.integers(-20, 21, size=3000))   # no batch at all: the same fold
    assert rt.bits(rt.final_fold(p, final="batch_descending")) == rt.bits(rt.final_fold(p))


def test_crosscheck_stats_place_by_hand():
    """Pixel (i, j) is thread i % 256 of part j * ceil(nrows / 256) + i / 256."""
    nrows, ncols = 300, 5
    mag = np.zeros((nrows, ncols))
    mag[0, 0], mag[1, 0], mag[3, 0] = BIG, 1.0, 1.0           # lanes 0, 1, 3 of part 0
    on = np.ones((nrows, ncols), bool)
    assert rt.crosscheck_stats(on, on, mag, nrows, ncols)["sum"] == BIG + 2.0
    mag[...] = 0.0
    mag[0, 0], mag[64, 0], mag[128, 0] = BIG, 1.0, 1.0        # waves 0, 1, 2 of part 0
    assert rt.crosscheck_stats(on, on, mag, nrows, ncols)["sum"] == BIG
    mag[...] = 0.0
    mag[299, 0], mag[0, 1], mag[256, 1] = BIG, 1.0, 1.0       # parts 1, 2, 3 = final lanes 1, 2, 3: (2^53 + 1) at d = 2, + 1 at d = 1
    got = rt.crosscheck_stats(on, on, mag, nrows, ncols)
    assert got["sum"] == BIG and got["nparts"] == 10 and got["defined"] == 1500 and got["max"] == BIG
    none = np.zeros((nrows, ncols), bool)
    got = rt.crosscheck_stats(none, none, np.full((nrows, ncols), np.nan), nrows, ncols)
    assert got["kept"] == 0 and got["defined"] == 0 and math.isnan(got["mean"]) and math.isnan(got["max"])


def test_flow_error_stats_order_by_hand():
    n = 3 * rt.ERR_TILE + 1
    on = np.ones(n, bool)

    def stats(**at):
        e = np.zeros(n)
        for k, x in at.items():
            e[int(k[1:])] = x
        return rt.flow_error_stats(on, e, e)

    assert stats(p7=BIG, p263=1.0, p519=1.0)["sum_epe"] == BIG            # one thread: its pixels t, t + 256, t + 512 in turn
    assert stats(p7=1.0, p263=1.0, p519=BIG)["sum_epe"] == BIG + 2.0
    assert stats(p0=BIG, p1=1.0, p3=1.0)["sum_ang"] == BIG + 2.0            # lanes 0, 1, 3
    assert stats(p0=BIG, p2048=1.0, p4096=1.0)["sum_epe"] == BIG           # tiles 0, 1, 2 in ascending order
    got = stats(p0=1.0, p2048=1.0, p6144=BIG)
    assert got["sum_epe"] == BIG + 2.0 and got["ntiles"] == 4 and got["count"] == n and got["max_epe"] == BIG
    e = np.zeros(n)
    e[0], e[2048], e[6144] = 1.0, 1.0, BIG
    assert rt.flow_error_stats(on, e, e, descending=True)["sum_epe"] == BIG
    # an uncounted pixel contributes nothing, whatever stands there
    e[5], off = np.nan, on.copy()
    off[5] = False
    got = rt.flow_error_stats(off, e, e)
    assert got["count"] == n - 1 and got["sum_epe"] == BIG + 2.0
    got = rt.flow_error_stats(np.zeros(n, bool), e, e)
    assert got["count"] == 0 and math.isnan(got["mean_epe"]) and math.isnan(got["mean_ang"]) and math.isnan(got["max_epe"])


@pytest.mark.parametrize("what", ("disp", "flow"))
def test_hand_cases(what):
    """2^53, 1, 1 in three parts of one final thread, in its order: the sum is 2^53, and 2^53 + 2 in any order in which the ones meet
    first -- inside the batch at 3073 parts, where the butterfly and the chain give the documented bits as well."""
    for ncols, parts in fc.HAND:
        ref, tree, mag = fc.hand_want(what, ncols, parts)
        live = 1 if what == "disp" else 2
        assert len({p % fc.FINAL_BLOCK for p in parts}) == 1 and tree["nparts"] == ncols
        assert ref["defined"] == 3 * live and ref["kept"] == ref["defined"] - 1 and ref["max"] == fc.HAND_BIG
        assert sorted(np.flatnonzero(ref["defined_mask"].any(axis=0))) == sorted(parts)
        assert tree["sum"] == fc.HAND_BIG and rt.bits(tree["mean"]) == rt.bits(fc.HAND_BIG / ref["defined"])
        assert rt.bits((fc.HAND_BIG + 2.0) / ref["defined"]) != rt.bits(tree["mean"])
    ncols, parts = fc.HAND[0]
    ref, tree, mag = fc.hand_want(what, ncols, parts)
    assert fc.final_iterations(ncols, 0) == (1, 0) and fc.final_iterations(ncols, 1) == (0, 3)
    wrong = rt.crosscheck_stats(ref["kept_mask"], ref["defined_mask"], mag, *mag.shape, final="batch_descending")
    assert wrong["sum"] == fc.HAND_BIG + 2.0
    assert fc.final_iterations(fc.HAND[1][0], 1023) == (1, 3) and fc.final_iterations(fc.HAND[2][0], 0) == (2, 1)


# ---- threads that hold nothing ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,shape", [("disp", (1, 4097)), ("flow", (2, 7169)), ("disp", (257, 1537)), ("flow", (513, 1366))])
def test_threads_that_hold_nothing_change_no_bit(what, shape):
    """The +0.0 of an undefined pixel's thread and of a thread below the plane replaced by -0.0, the one value whose addition leaves
    every other value's bits alone: the same statistics.  (The sums are non-negative, so +0.0 is as good.)"""
    ref, tree, mag = fc.cross_want(what, shape, "binades")
    k, d, s, m = rt.crosscheck_thread_values(ref["kept_mask"], ref["defined_mask"], mag, *shape)
    dead = d == 0.0
    assert dead.sum() == d.size - ref["defined"] and dead.sum() > shape[1] * (-shape[0] % 256)
    assert np.all(m[dead] == -1.0) and np.all(s[dead] == 0.0) and not np.signbit(s[dead]).any() and np.all(k[dead] == 0.0)
    quiet = s.copy()
    quiet[dead] = -0.0
    assert rt.bits(rt.final_fold(rt.workgroup_fold(quiet))) == rt.bits(tree["sum"]) == rt.bits(rt.final_fold(rt.workgroup_fold(s)))
    assert rt.final_fold(rt.workgroup_fold(m, True), True) == tree["max"] == mag[ref["defined_mask"]].max()


# ---- the binades cases tell the orders apart -------------------------------------------------------------------------------------
def cross_means(what, shape):
    """The restated mean of the binades case and the three means it must not have the bits of."""
    ref, tree, mag = fc.cross_want(what, shape, "binades")
    masks = ref["kept_mask"], ref["defined_mask"]
    chain = rt.crosscheck_stats(*masks, mag, *shape, final="chain")["mean"]
    backwards = rt.crosscheck_stats(*masks, mag, *shape, steps=REVERSED)["mean"]
    wrong = [ref["mean"], chain, backwards]
    if fc.final_iterations(fc.nparts_of(shape), 1023)[0]:   # every thread runs a batch: each batch of four folded last part first
        wrong.append(rt.crosscheck_stats(*masks, mag, *shape, final="batch_descending")["mean"])
    return (tree["mean"],) + tuple(wrong)


@pytest.mark.parametrize("what,shape", CROSS, ids=[cross_id(c) for c in CROSS])
def test_binades_cross_cases_pin_the_order(what, shape):
    ref, tree, mag = fc.cross_want(what, shape, "binades")
    n = shape[0] * shape[1]
    assert n - 30 <= ref["defined"] < n and 0.4 * n < ref["kept"] < 0.6 * n
    assert tree["kept"] == ref["kept"] and tree["defined"] == ref["defined"] and rt.bits(tree["max"]) == rt.bits(ref["max"])
    mean, fsum, *others = cross_means(what, shape)
    assert len(others) == (3 if fc.nparts_of(shape) >= 4 * fc.FINAL_BLOCK else 2)
    assert abs(mean - fsum) <= 2.0 * ref["defined"] * 2.0 ** -53 * fsum
    assert rt.bits(mean) not in [rt.bits(x) for x in [fsum] + others], "reseed (%r, %r) in flow_round_cases.RESEED" % (what, shape)


def error_means(case):
    """The flow errors' final pass is itself one ascending chain, so the third wrong order here is the descending one."""
    ref, tree = fc.error_want(case)
    flat = lambda a: a.reshape(-1, order="F")
    planes = flat(ref["counted"]), flat(ref["epe_plane64"]), flat(ref["ang_plane64"])
    return (tree["mean_epe"], ref["mean_epe"], rt.flow_error_stats(*planes, descending=True)["mean_epe"],
            rt.flow_error_stats(*planes, steps=REVERSED)["mean_epe"])


@pytest.mark.parametrize("case", [c for c in fc.error_cases() if c[1] == "binades"], ids=fc.error_id)
def test_binades_error_cases_pin_the_order(case):
    ref, tree = fc.error_want(case)
    assert tree["count"] == ref["count"] and rt.bits(tree["max_epe"]) == rt.bits(ref["max_epe"])
    mean, fsum, descending, backwards = error_means(case)
    assert abs(mean - fsum) <= 2.0 * ref["count"] * 2.0 ** -53 * fsum
    assert rt.bits(mean) not in (rt.bits(fsum), rt.bits(descending), rt.bits(backwards)), "reseed %r in flow_round_cases.RESEED" % (case,)
