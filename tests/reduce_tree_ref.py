"""The library's fixed-order float64 sums, restated in NumPy for the statistics of the cross-checks (k_disp_crosscheck,
k_flow_crosscheck, k_crosscheck_final; csrc/pdeip_crosscheck.hpp) and of the flow errors (k_flow_err_tiles, k_flow_err_final;
csrc/pdeip_flowviz.hpp): plain float64, one rounded addition per step, in exactly the order the kernel comments give.

  wave_tree        v = v + v[lane ^ d] for d = 32, 16, 8, 4, 2, 1 over the 64 lanes; lane 0 (every lane ends with the same bits)
  workgroup_fold   wave_tree of each of the four waves, then the waves in ascending order
  crosscheck_stats one value per thread of the pixel grid, workgroup_fold per part, final thread t folds parts t, t + 1024, .. in
                   ascending order, wave_tree, the sixteen waves in ascending order
  flow_error_stats a thread's 8 pixels in ascending order (an uncounted pixel adds nothing, not +0.0), workgroup_fold per tile, the
                   tiles in ascending order from 0.0 (from -1 for the maximum)

Every sequential fold here is an explicit loop or np.add.accumulate, which must form each prefix in turn.  np.sum and np.add.reduce
add pairwise (in blocks of eight accumulators) and give another order, hence other bits: they are not used on anything whose order
matters.  The maxima use > against the sentinel -1 as the kernels do; a maximum is exact in any order.

`steps` and `final` select deliberately wrong orders.  tests/test_reduce_tree_ref.py uses them to prove that a case can tell the
documented order from another one; no GPU comparison uses anything but the defaults."""
import math

import numpy as np

F64 = np.float64
WAVE, BLOCK, FINAL_BLOCK, ERR_PER_THREAD = 64, 256, 1024, 8
ERR_TILE = BLOCK * ERR_PER_THREAD
STEPS = (32, 16, 8, 4, 2, 1)


def _partner(v, d):
    """v[..., lane ^ d]: the lanes in groups of 2 d, the two halves of each group exchanged."""
    w = v.reshape(v.shape[:-1] + (WAVE // (2 * d), 2, d))
    return w[..., ::-1, :].reshape(v.shape)


def wave_tree(v, steps=STEPS):
    """The butterfly sum of v[..., 64] -> [...]."""
    v = np.asarray(v, F64)
    assert v.shape[-1] == WAVE
    for d in steps:
        v = v + _partner(v, d)
    return v[..., 0]


def wave_tree_max(v, steps=STEPS):
    v = np.asarray(v, F64)
    assert v.shape[-1] == WAVE
    for d in steps:
        other = _partner(v, d)
        v = np.where(other > v, other, v)
    return v[..., 0]


def _waves_ascending(w, maximum):
    """w[..., nwaves]: wave 0's value, then waves 1, 2, .. folded onto it in turn."""
    acc = w[..., 0]
    for k in range(1, w.shape[-1]):
        acc = np.where(w[..., k] > acc, w[..., k], acc) if maximum else acc + w[..., k]
    return acc


def workgroup_fold(vals, maximum=False, steps=STEPS):
    """vals[..., 64 w]: one value per thread of a workgroup of w waves -> [...]: wave_tree, then the waves in ascending order."""
    vals = np.asarray(vals, F64)
    w = vals.reshape(vals.shape[:-1] + (vals.shape[-1] // WAVE, WAVE))
    return _waves_ascending(wave_tree_max(w, steps) if maximum else wave_tree(w, steps), maximum)


def chain(values, start=0.0):
    """start + values[0] + values[1] + ..: a single chain in ascending order."""
    return float(np.add.accumulate(np.concatenate([[start], np.asarray(values, F64)]))[-1])


def crosscheck_thread_values(kept, defined, mag, nrows, ncols):
    """-> kept, defined, sum, largest as [nparts, 256]: one row per workgroup of pixel_grid(nrows, ncols, 1), part = col *
    ceil(nrows / 256) + rowblock.  A thread with i >= nrows and a thread whose pixel is not defined hold 0, 0, 0, -1."""
    kept, defined = np.asarray(kept, bool).reshape(nrows, ncols), np.asarray(defined, bool).reshape(nrows, ncols)
    mag = np.asarray(mag, F64).reshape(nrows, ncols)
    blocks = (nrows + BLOCK - 1) // BLOCK
    out = []
    for plane in (np.where(defined & kept, 1.0, 0.0), np.where(defined, 1.0, 0.0), np.where(defined, mag, 0.0), np.where(defined, mag, -1.0)):
        t = np.zeros((ncols, blocks * BLOCK), F64) if len(out) < 3 else np.full((ncols, blocks * BLOCK), -1.0)
        t[:, :nrows] = plane.T
        out.append(t.reshape(ncols * blocks, BLOCK))
    return out


def crosscheck_partials(kept, defined, mag, nrows, ncols, steps=STEPS):
    """The four rows of the partials, [4][nparts]."""
    k, d, s, m = crosscheck_thread_values(kept, defined, mag, nrows, ncols)
    return [workgroup_fold(k, steps=steps), workgroup_fold(d, steps=steps), workgroup_fold(s, steps=steps), workgroup_fold(m, True, steps)]


def _threads_batch_descending(parts, batch=4):
    """The final threads' sums with the loops of k_crosscheck_final as they stand -- thread t takes `batch` parts at a time while
    p < nparts - (batch - 1) * 1024, the rest one at a time -- but each batch folded last part first (a wrong order)."""
    n = parts.size
    rounds = (n + FINAL_BLOCK - 1) // FINAL_BLOCK
    P = np.zeros(rounds * FINAL_BLOCK)
    P[:n] = parts
    P = P.reshape(rounds, FINAL_BLOCK)
    live = (np.arange(rounds * FINAL_BLOCK) < n).reshape(rounds, FINAL_BLOCK)
    t = np.arange(FINAL_BLOCK)
    acc, batched = np.zeros(FINAL_BLOCK), np.ones(FINAL_BLOCK, bool)
    for r0 in range(0, rounds, batch):
        batched = batched & (r0 * FINAL_BLOCK + t < n - (batch - 1) * FINAL_BLOCK)
        for r in range(min(r0 + batch, rounds) - 1, r0 - 1, -1):
            acc = np.where(batched, acc + P[r], acc)
        for r in range(r0, min(r0 + batch, rounds)):
            acc = np.where(~batched & live[r], acc + P[r], acc)
    return acc


def final_fold(parts, maximum=False, steps=STEPS, final="strided"):
    """k_crosscheck_final on one row of the partials.  final 'chain': one thread, every part in ascending order; 'batch_descending':
    each batch of four folded last part first (two wrong orders)."""
    parts = np.asarray(parts, F64)
    if final == "chain":
        return float(parts.max(initial=-1.0)) if maximum else chain(parts)
    if final == "batch_descending":
        return float(workgroup_fold(_threads_batch_descending(parts), False, steps))
    acc = np.full(FINAL_BLOCK, -1.0 if maximum else 0.0)
    for base in range(0, parts.size, FINAL_BLOCK):   # thread t: parts t, t + 1024, .. in ascending order
        seg = parts[base:base + FINAL_BLOCK]
        head = acc[:seg.size]
        acc[:seg.size] = np.where(seg > head, seg, head) if maximum else head + seg
    return float(workgroup_fold(acc, maximum, steps))


def crosscheck_stats(kept, defined, mag, nrows, ncols, steps=STEPS, final="strided"):
    """-> dict kept, defined, sum, mean, max of pdeip_*_crosscheck's stats_out; NaN mean and max with nothing defined."""
    pk, pd, ps, pm = crosscheck_partials(kept, defined, mag, nrows, ncols, steps)
    k, d, s, m = (final_fold(pk, False, steps, final), final_fold(pd, False, steps, final), final_fold(ps, False, steps, final),
                  final_fold(pm, True, steps, final))
    with np.errstate(invalid="ignore"):
        mean = float(F64(s) / F64(d))
    return dict(kept=k, defined=d, sum=s, mean=mean, max=m if d > 0.0 else math.nan, nparts=pk.size)


def flow_error_partials(counted, epe, ang, steps=STEPS):
    """counted, epe, ang: one entry per pixel in memory (column-major) order -> the tile partials [4][ntiles]: count, sum of endpoint
    errors, sum of angular errors, largest endpoint error (-1: none)."""
    counted = np.asarray(counted, bool).ravel()
    n = counted.size
    ntiles = (n + ERR_TILE - 1) // ERR_TILE
    c = np.zeros(ntiles * ERR_TILE, bool)
    c[:n] = counted
    c = c.reshape(ntiles, ERR_PER_THREAD, BLOCK)   # pixel tile * 2048 + k * 256 + t
    planes = []
    for x in (epe, ang):
        p = np.zeros(ntiles * ERR_TILE, F64)
        p[:n] = np.where(counted, np.asarray(x, F64).ravel(), 0.0)
        planes.append(p.reshape(ntiles, ERR_PER_THREAD, BLOCK))
    cnt, se, sa, me = np.zeros((ntiles, BLOCK)), np.zeros((ntiles, BLOCK)), np.zeros((ntiles, BLOCK)), np.full((ntiles, BLOCK), -1.0)
    for k in range(ERR_PER_THREAD):   # a pixel that is not counted adds nothing
        on = c[:, k, :]
        cnt = np.where(on, cnt + 1.0, cnt)
        se = np.where(on, se + planes[0][:, k, :], se)
        sa = np.where(on, sa + planes[1][:, k, :], sa)
        me = np.where(on & (planes[0][:, k, :] > me), planes[0][:, k, :], me)
    return [workgroup_fold(cnt, steps=steps), workgroup_fold(se, steps=steps), workgroup_fold(sa, steps=steps), workgroup_fold(me, True, steps)]


def flow_error_stats(counted, epe, ang, steps=STEPS, descending=False):
    """-> dict count, mean_epe, mean_ang, max_epe of pdeip_flow_errors' stats_out.  descending: the tiles folded last to first (a
    wrong order)."""
    pc, pe, pa, pm = flow_error_partials(counted, epe, ang, steps)
    order = slice(None, None, -1) if descending else slice(None)
    cnt, se, sa = chain(pc[order]), chain(pe[order]), chain(pa[order])
    largest = -1.0
    for v in pm[order]:
        if v > largest:
            largest = float(v)
    with np.errstate(invalid="ignore"):
        return dict(count=cnt, sum_epe=se, sum_ang=sa, mean_epe=float(F64(se) / F64(cnt)), mean_ang=float(F64(sa) / F64(cnt)),
                    max_epe=largest if cnt > 0.0 else math.nan, ntiles=pc.size)


def bits(x):
    return int(np.float64(x).view(np.uint64))
