"""CPU: the masks of tests/ccl_edge_cases.py are what they claim.  The flood fill equals scipy.ndimage.label on each; the area
table's hash and probe, the block and round counts and the chunk carry of k_ccl_small are restated here in plain Python from the
constants of csrc/pdeip_ccl_plan.hpp / pdeip_ccl.hpp, and the cases are shown to reach what they were built to reach.  These are
conditions on the inputs: if an edit to a case breaks one, this file fails, not the GPU test."""
import functools

import numpy as np
import pytest
from scipy import ndimage

import ccl_cases
import ccl_edge_cases as ec
import ccl_ref

LIN_PIX, HASH_SLOTS, HASH_MUL, HASH_SHIFT = 1024, 2048, 2654435761, 21
SCAN_THREADS, ARG_THREADS, CHUNK = 256, 1024, 64


@functools.lru_cache(maxsize=None)
def lab(name, conn):
    out = ccl_ref.label(ec.get(name), conn)
    for a in (out[0], out[2]):
        a.setflags(write=False)
    return out


# ---- the restatements ----------------------------------------------------------------------------------------------------------
def slot_of(key):
    return ((int(key) * HASH_MUL) & 0xFFFFFFFF) >> HASH_SHIFT


def table_stats(L):
    """area_table_add over the labels of each LIN_PIX pixels in memory order, each label inserted where it first appears:
    (insertions that found their slot taken, the longest probe in slots, probes that stepped from the last slot to slot 0, those
    of them that found slot 0 taken as well)."""
    flat = np.asarray(L).T.ravel()
    collided = longest = wraps = wraps_onto_taken = 0
    for base in range(0, flat.size, LIN_PIX):
        blk = flat[base:base + LIN_PIX]
        blk = blk[blk > 0]
        keys = blk[np.sort(np.unique(blk, return_index=True)[1])]
        taken = set()
        for key in keys:
            slot, probe = slot_of(key), 0
            while slot in taken:
                nxt = (slot + 1) & (HASH_SLOTS - 1)
                if nxt < slot:
                    wraps += 1
                    wraps_onto_taken += nxt in taken
                slot, probe = nxt, probe + 1
            taken.add(slot)
            collided += probe > 0
            longest = max(longest, probe)
    return collided, longest, wraps, wraps_onto_taken


def blocks_and_rounds(A):
    blocks = -(-A.size // LIN_PIX)
    return blocks, -(-blocks // SCAN_THREADS)


def small_run_starts(fg):
    """Step 1 of k_ccl_small: (the row every foreground pixel points at, -1 elsewhere; the (column, chunk's first row, carry) of
    every chunk that is foreground throughout and keeps a carry from the chunk above)."""
    rows, cols = fg.shape
    start = np.full(fg.shape, -1, int)
    kept = []
    for j in range(cols):
        carry = -1
        for i0 in range(0, rows, CHUNK):
            bal = np.zeros(CHUNK, bool)
            n = min(CHUNK, rows - i0)
            bal[:n] = fg[i0:i0 + n, j]
            for lane in range(n):
                below = np.flatnonzero(~bal[:lane])
                st = i0 + below[-1] + 1 if below.size else (carry if carry >= 0 else i0)
                if bal[lane]:
                    start[i0 + lane, j] = st
            if bal[CHUNK - 1]:
                z = np.flatnonzero(~bal)
                if z.size:
                    carry = i0 + z[-1] + 1
                else:
                    if carry >= 0:
                        kept.append((j, i0, carry))
                    carry = carry if carry >= 0 else i0
            else:
                carry = -1
    return start, kept


def true_run_starts(fg):
    start = np.full(fg.shape, -1, int)
    for j in range(fg.shape[1]):
        s = -1
        for i in range(fg.shape[0]):
            s = (i if s < 0 else s) if fg[i, j] else -1
            start[i, j] = s
    return start


def covers_a_chunk(a, b):
    return any(a <= i0 and i0 + CHUNK - 1 <= b for i0 in range(0, ec.CARRY_ROWS - CHUNK + 1, CHUNK))


# ---- every case against scipy ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("name", ec.names())
def test_flood_fill_equals_scipy_on_the_transposed_mask(name, conn):
    A = ec.get(name)
    L, num, areas = lab(name, conn)
    want, n = ndimage.label(ccl_ref.foreground(A).T, structure=np.ones((3, 3), int) if conn == 8 else None)
    assert num == n
    assert np.array_equal(L, want.T)
    assert np.array_equal(areas, np.bincount(want.ravel(), minlength=n + 1)[1:])
    assert L.dtype == np.int32 and areas.dtype == np.int32


def test_names_are_unique_planes_read_only_and_within_the_flood_fill_budget():
    names = ec.names()
    assert len(set(names)) == len(names) and not set(names) & set(ccl_cases.names())
    for name, A in ec.cases():
        assert A.dtype == np.float32 and A.flags.c_contiguous and not A.flags.writeable, name
        assert int((A > 0).sum()) <= 150000, name
        assert ccl_cases.get(name) is A  # the lookup the GPU tests' reference() goes through


# ---- a. the small form's limits --------------------------------------------------------------------------------------------------
def test_small_limit_cases_have_the_pixel_counts_named():
    assert ccl_cases.SMALL_MAX_PIX == 16384
    for shape in ec.SMALL_LIMIT_SHAPES:
        for kind in ("fg", "r50", "alt"):
            A = ec.get("small_%dx%d_%s" % (shape + (kind,)))
            assert A.shape == shape and ec.admits_small(A)
            assert A.size == (16383 if 127 in shape else 16384)  # at the limit, or one pixel under it with odd rows and columns
        assert ec.get("small_%dx%d_fg" % shape).all()
        alt = ec.get("small_%dx%d_alt" % shape).T.ravel()
        assert alt[0::2].all() and not alt[1::2].any()
    past = ec.get("past_%dx%d_r50" % ec.PAST_LIMIT_SHAPE)
    assert past.size == 16385 and not ec.admits_small(past)
    assert lab("small_128x128_checker", 4)[1] == 8192 and lab("small_128x128_checker", 8)[1] == 1  # the most labels the form can meet
    assert lab("small_16384x1_alt", 8)[1] == 8192 and lab("small_1x16384_alt", 8)[1] == 8192


def test_patterns_fit_the_small_form_and_span_the_chunks_named():
    for shape, chunks in ((ec.PATTERN_SHAPE_2, 2), (ec.PATTERN_SHAPE_4, 4)):
        assert shape[0] * shape[1] <= 16384 and -(-shape[0] // CHUNK) == chunks
    r, c = ec.PATTERN_SHAPE_2
    for name in ("serpentine", "spiral", "comb_last_row", "comb_first_row", "comb_last_col", "comb_first_col"):
        A = ec.get("%s_%dx%d" % (name, r, c))
        assert A.shape == (r, c) and lab("%s_%dx%d" % (name, r, c), 4)[1] == 1
    for name in ("diag_plus", "diag_minus"):
        A = ec.get("%s_%dx%d" % (name, r, c))
        assert lab("%s_%dx%d" % (name, r, c), 4)[1] == int((A > 0).sum())
    r, c = ec.PATTERN_SHAPE_4
    for name in ("serpentine", "comb_last_row", "comb_first_row"):
        A = ec.get("%s_%dx%d" % (name, r, c))
        assert lab("%s_%dx%d" % (name, r, c), 4)[1] == 1
        start, kept = small_run_starts(A > 0)
        assert np.array_equal(start, true_run_starts(A > 0))
        # a full column keeps its carry through the two whole middle chunks
        assert {(i0, carry) for j, i0, carry in kept if j == 0} == {(64, 0), (128, 0)}
        assert len(kept) >= 2 * (c // 2)


def test_carry_cases_hold_every_pair_and_every_whole_chunk_run_fits_the_small_form():
    assert len(ec.CARRY_PAIRS) == 136
    names = [n for n in ec.names() if n.startswith("carry_")]
    seen_small, seen_all, kept_small = set(), set(), set()
    for name in names:
        A = ec.get(name)
        fg = A > 0
        assert A.shape[0] == ec.CARRY_ROWS
        start, kept = small_run_starts(fg)
        assert np.array_equal(start, true_run_starts(fg)), name
        pairs = []
        for j in range(A.shape[1]):
            rows = np.flatnonzero(fg[:, j])
            if j % 2:
                assert rows.size == 0  # a background column between two runs
                continue
            assert np.array_equal(rows, np.arange(rows[0], rows[-1] + 1))  # one run
            pairs.append((int(rows[0]), int(rows[-1])))
        for conn in (4, 8):  # the closed form: run k is component k + 1
            L, num, areas = lab(name, conn)
            assert num == len(pairs) and [int(a) for a in areas] == [b - a + 1 for a, b in pairs]
            assert all(L[a, 2 * k] == k + 1 and L[b, 2 * k] == k + 1 for k, (a, b) in enumerate(pairs))
        if name == "carry_all":
            assert not ec.admits_small(A)
            seen_all |= set(pairs)
        else:
            assert ec.admits_small(A)
            seen_small |= set(pairs)
            kept_small |= {(carry, i0) for _, i0, carry in kept}
    assert seen_all == set(ec.CARRY_PAIRS) and seen_small == set(ec.CARRY_PAIRS)
    assert {p for p in ec.CARRY_PAIRS if covers_a_chunk(*p)} <= seen_small
    # the branch that keeps a carry across a whole chunk, with every start and at every chunk the pairs allow
    want = {(a, i0) for a, b in ec.CARRY_PAIRS for i0 in range(CHUNK, ec.CARRY_ROWS, CHUNK) if a < i0 and i0 + CHUNK - 1 <= b}
    assert kept_small == want and len(want) >= 20
    assert any(b - a >= 3 * CHUNK for a, b in seen_small)  # three whole chunks in one run


# ---- b. seams and corners ---------------------------------------------------------------------------------------------------------
def test_seam_planes_have_the_sizes_named():
    for rows in ec.SEAM_ROWS:
        for cols in ec.SEAM_COLS:
            assert ec.get("seam_%dx%d_fg" % (rows, cols)).all() and ec.get("seam_%dx%d_fg" % (rows, cols)).shape == (rows, cols)
            r = ec.get("seam_%dx%d_r50" % (rows, cols))
            assert r.shape == (rows, cols) and 0.4 < r.mean() < 0.6
    assert any(r % ec.TILE_I == 0 and c % ec.TILE_J == 0 for r in ec.SEAM_ROWS for c in ec.SEAM_COLS)  # exact tile multiples


def _components_2x2(pattern, conn):
    m = np.zeros((2, 2), np.float32)
    for bit, (di, dj) in enumerate(ec.CORNER_PIXELS):
        m[1 + di, 1 + dj] = pattern >> bit & 1
    return ccl_ref.label(m, conn)[1]


def test_every_corner_pattern_sits_at_a_four_tile_corner():
    places = ec.corner_places()
    assert len(places) == 25 and all(i0 % ec.TILE_I == 0 and j0 % ec.TILE_J == 0 and i0 > 0 and j0 > 0 for i0, j0 in places)
    plain, arms = ec.get("corners_330x170") > 0, ec.get("corner_arms_330x170") > 0
    seen = [sum(int(plain[i0 + di, j0 + dj]) << bit for bit, (di, dj) in enumerate(ec.CORNER_PIXELS)) for i0, j0 in places]
    assert set(seen) == set(range(16))
    assert seen == [sum(int(arms[i0 + di, j0 + dj]) << bit for bit, (di, dj) in enumerate(ec.CORNER_PIXELS)) for i0, j0 in places]
    bits = sum(bin(p).count("1") for p in seen)
    assert int(plain.sum()) == bits and int(arms.sum()) == 3 * bits  # nothing else on the planes
    # num says which adjacencies across the corner were merged: the anti-diagonal (i0-1, j0)-(i0, j0-1) is pattern 6, the diagonal 9
    assert _components_2x2(6, 8) == 1 and _components_2x2(6, 4) == 2 and _components_2x2(9, 8) == 1 and _components_2x2(9, 4) == 2
    for conn in (4, 8):
        assert lab("corners_330x170", conn)[1] == sum(_components_2x2(p, conn) for p in seen)
    assert lab("corner_arms_330x170", 8)[1] == lab("corners_330x170", 8)[1]
    assert lab("corner_arms_330x170", 4)[1] == lab("corners_330x170", 4)[1] + 2 * bits


def test_seam_patterns_hold_every_neighbourhood_away_from_the_corners():
    for kind, name, offsets in (("col", "seam_patterns_col32", ec.SEAM_WEST), ("row", "seam_patterns_row64", ec.SEAM_NORTH)):
        fg = ec.get(name) > 0
        shape, places = ec.seam_pattern_places(kind)
        assert fg.shape == shape and len(places) == 32
        seen = set()
        for i, j in places:
            assert fg[i, j] and (j == ec.TILE_J if kind == "col" else i == ec.TILE_I)
            along, crossing = (i, range(ec.TILE_I, shape[0], ec.TILE_I)) if kind == "col" else (j, range(ec.TILE_J, shape[1], ec.TILE_J))
            assert all(abs(along - s) > 3 for s in crossing)  # no corner within the neighbourhood
            seen.add(sum(int(fg[i + di, j + dj]) << bit for bit, (di, dj) in enumerate(offsets)))
        assert seen == set(range(32))
        assert int(fg.sum()) == 32 + 5 * 16  # nothing else on the plane


# ---- c. the scan's rounds and the far side of the argmax ------------------------------------------------------------------------
def test_scan_cases_have_the_block_counts_named_and_roots_at_both_ends():
    rounds = {}
    for blocks, shape in ec.SCAN_SHAPES.items():
        name = "lattice_%dx%d_%dblocks" % (shape + (blocks,))
        A = ec.get(name)
        assert blocks_and_rounds(A)[0] == blocks and not ec.admits_small(A)
        rounds[blocks] = blocks_and_rounds(A)[1]
        for conn in (4, 8):
            L, num, areas = lab(name, conn)
            assert L[0, 0] == 1 and L[-1, -1] == num and areas[num - 1] == 1  # a root in the first block and one in the last
            assert num == int((A > 0).sum()) and num > 2 * ARG_THREADS
            per_block = np.bincount(np.flatnonzero(L.T.ravel() > 0) // LIN_PIX, minlength=blocks)
            assert all(per_block[r:r + SCAN_THREADS].sum() > 0 for r in range(0, blocks, SCAN_THREADS))  # roots in every round
    assert rounds == {256: 1, 257: 2, 512: 2, 513: 3}
    old = max(blocks_and_rounds(A)[0] for _, A in ccl_cases.cases())
    assert old == 384  # what the first list reaches: two rounds, never a full one followed by a block


def test_far_cases_tie_or_win_on_the_far_side_of_the_stride():
    for n, beyond in ((80, ARG_THREADS), (160, 2 * ARG_THREADS)):
        A = ec.get("largest_far_tie_%dx%d" % (n, n))
        assert ec.admits_small(A) == (n == 80)
        for conn in (4, 8):
            areas = lab("largest_far_tie_%dx%d" % (n, n), conn)[2]
            top = np.flatnonzero(areas == areas.max()) + 1
            assert len(top) == 2 and top[0] <= ARG_THREADS and top[1] > beyond and areas.max() == 3
            assert np.sort(areas)[-3] == 1  # equal areas that exceed every other area
            sel = ccl_ref.largest_component(A, conn, 5.0, -5.0)[0]
            L = lab("largest_far_tie_%dx%d" % (n, n), conn)[0]
            assert (sel[L == top[0]] == 5.0).all() and (sel[L == top[1]] == -5.0).all()  # the lower label wins
        for conn in (4, 8):
            areas = lab("largest_far_unique_%dx%d" % (n, n), conn)[2]
            top = np.flatnonzero(areas == areas.max()) + 1
            assert len(top) == 1 and top[0] > beyond and areas.max() == 3


# ---- d. the area table ---------------------------------------------------------------------------------------------------------------
def test_the_hash_constants_put_the_named_labels_in_the_last_and_the_first_slot():
    assert [k for k in range(1, 7000) if slot_of(k) == HASH_SLOTS - 1] == [987, 2584, 5168, 6765]
    assert [k for k in range(1, 5000) if slot_of(k) == 0] == [1597, 4181]
    assert len({slot_of(k) for k in range(1, 513)}) == 512  # consecutive labels spread perfectly: the checkerboard never collides


def test_rake_cases_collide_in_the_area_table():
    for shape in ec.RAKE_SHAPES:
        collided, longest, _, _ = table_stats(lab("rake_%dx%d" % shape, 8)[0])
        assert collided >= 100 and longest >= 2, (shape, collided, longest)


def test_wrap_case_probes_from_the_last_slot_onto_a_taken_first_slot():
    A = ec.get("wrap_%dx%d" % ec.WRAP_SHAPE)
    starts = ec.wrap_plane()[1]
    for conn in (4, 8):
        L, num, areas = lab("wrap_%dx%d" % ec.WRAP_SHAPE, conn)
        assert (L[0, starts[0]], L[-1, starts[1]]) == ec.WRAP_LINE_LABELS
        assert areas[986] == A.shape[1] - starts[0] and areas[1596] == A.shape[1] - starts[1] and num > 6765
        collided, longest, wraps, onto_taken = table_stats(L)
        assert wraps >= 3 and onto_taken >= 3 and longest >= 2, (collided, longest, wraps, onto_taken)
        flat = L.T.ravel()
        for late in (2584, 5168, 6765):  # each meets both lines in its block
            blk = flat[np.flatnonzero(flat == late)[0] // LIN_PIX * LIN_PIX:][:LIN_PIX]
            assert 987 in blk and 1597 in blk
