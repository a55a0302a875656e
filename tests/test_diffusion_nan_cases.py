"""CPU: every case of tests/diffusion_nan_cases.py is what it claims, and the DdiffWeights oracle keeps the gateway's rule at NaN.

The GPU tests (test_gpu_diffusion_nan.py) only consume the cases.  What a diffusion case contains -- where its non-finite outputs
lie, that the channels it leaves alone stay finite (so that a comparison in which any NaN equals any NaN still proves something),
and whether the .m's maximum and the gateway's part on it -- is proved here from the numpy restatement alone.  The gateway cases pin
the project's C oracle to the reference's own compiled DdiffWeights and both to a numpy statement of its first-frame-sticky rule."""
import numpy as np
import pytest

import diffusion_nan_cases as dc
import diffusion_ref as ref
import problems as pb
import ref_lib
from test_diffusion import _require_ref_build

F32 = np.float32


def _eq(got, want, what):
    assert pb.bit_equal(got, want), "%s: %s" % (what, pb.describe_mismatch(got, want))


# ---- the two rules -------------------------------------------------------------------------------------------------------------

def test_the_two_maxima_part_only_at_a_nan_of_frame_0():
    nan, inf = np.nan, np.inf
    T = np.array([[1, 2, 3], [3, 2, 1], [2, 2, 2], [nan, 1, 2], [1, nan, 0.5], [1, 2, nan], [nan, nan, 3], [nan, nan, nan],
                  [inf, nan, 1], [nan, inf, 1], [1, inf, nan], [0, 0, 0]], F32)
    omit = np.fmax.reduce(T, axis=1)
    sticky = dc.sticky_max(T)
    assert np.array_equal(omit[:3], [3, 3, 2]) and np.array_equal(sticky[:3], [3, 3, 2])
    assert omit[3:].tolist()[:4] == [2, 1, 2, 3] and np.isnan(omit[7])
    assert np.isnan(sticky[[3, 6, 7, 9]]).all() and sticky[[4, 5]].tolist() == [1, 2]
    assert omit[8:].tolist() == [inf, inf, inf, 0] and sticky[[8, 10, 11]].tolist() == [inf, inf, 0]
    same = [pb.bit_equal(a, b) for a, b in zip(omit, sticky)]
    assert same == [not (np.isnan(t[0]) and not np.isnan(t).all()) for t in T]


# ---- the diffusion cases -------------------------------------------------------------------------------------------------------

def test_diffusion_cases_cover_the_placements():
    single = [dc.CASES[n] for n in dc.SINGLE]
    assert {c.shape for c in single} == {(12, 70, 3), (66, 9, 2), (258, 66, 4), (3, 3, 3), (2, 2, 2)}
    for C in (2, 3, 4):
        of_c = [c for c in single if c.shape[2] == C]
        for v in dc.VALUES:
            chans = {c.lace[0][2] for c in of_c if c.lace[0][3] == v}
            assert {0, C - 1} <= chans and (C == 2 or chans & set(range(1, C - 1))), (C, v)
    where = {(c.shape, c.lace[0][:2]) for c in single}
    for shape in ((12, 70, 3), (66, 9, 2), (258, 66, 4)):
        assert {(shape, (0, 0)), (shape, (shape[0] - 1, shape[1] - 1))} <= where
    rows = {(s, p[0]) for s, p in where}
    cols = {(s, p[1]) for s, p in where}
    assert {((66, 9, 2), 63), ((66, 9, 2), 64), ((258, 66, 4), 63), ((258, 66, 4), 64), ((258, 66, 4), 255), ((258, 66, 4), 256)} <= rows
    assert {((12, 70, 3), 63), ((12, 70, 3), 64), ((258, 66, 4), 63), ((258, 66, 4), 64)} <= cols
    # every single-pixel case at one and at two iterations, the all-NaN channel at six as well
    assert {c.outer_iter for c in single} == {0, 1}
    assert all(n.replace("-iter0", "-iter1") in dc.CASES for n in dc.SINGLE if n.endswith("-iter0"))
    assert [ref.iterations(k) for k in (0, 1, 5)] == [1, 2, 6]
    assert {c.outer_iter for c in dc.CASES.values() if "channel0_all_nan" in c.name} == {0, 1, 5}
    assert set(dc.QUOTED) <= set(dc.NAMES)
    both = {c.differs for c in dc.CASES.values()}
    assert both == {True, False}


@pytest.mark.parametrize("name", dc.NAMES)
def test_diffusion_case_is_what_it_claims(name):
    case, I, out = dc.CASES[name], dc.laced(name), dc.want(name)
    assert I.shape == case.shape and I.dtype == F32 and not I.flags.writeable and out.shape == case.shape
    # the lacing: exactly the named pixels are non-finite, with the named values
    bad = np.zeros(case.shape, bool)
    for i, j, c, v in case.lace:
        at = (slice(None) if i is None else i, slice(None) if j is None else j, c)
        bad[at] = True
        assert np.array_equal(np.asarray(I[at]).view(np.uint32).ravel()[:1], np.asarray(dc.VALUES[v], F32).view(np.uint32).ravel()), v
    assert np.array_equal(~np.isfinite(I), bad)
    # uint8 has NaN to turn into 0, and there are bits to compare -- but for the one flood: NaN in every channel gives NaN weights
    # along the pixel's row and column in the second iteration, which every line crosses
    assert np.isnan(out).any() and np.isfinite(out).any() == (name != dc.FLOOD)
    # the channels the case leaves alone come back finite after every iteration count: the .m's maximum drops what is not a number
    for k in range(case.shape[2]):
        if k not in dc.touched(case):
            assert np.isfinite(out[:, :, k]).all(), "channel %d" % k
    if case.single:
        assert bad.sum() == 1
        (i, j, c, _), = case.lace
        if ref.iterations(case.outer_iter) == 1:  # the pixel's row and column in its own channel, all of both and nothing else
            line = np.zeros(case.shape, bool)
            line[i, :, c] = True
            line[:, j, c] = True
            assert np.array_equal(~np.isfinite(out), line)
    # the two rules part exactly where the case says so: the GPU test of a case that differs fails for a kernel with the gateway's rule
    sticky = dc.want_sticky(name)
    assert pb.bit_equal(out, sticky) == (not case.differs), (dc.finite_share(out), dc.finite_share(sticky))
    if case.differs:
        assert np.isnan(sticky[:, :, 1:]).any()  # the gateway's rule lets channel 0 into the others


@pytest.mark.parametrize("name", sorted(dc.QUOTED))
def test_finite_shares_by_which_the_cases_were_chosen(name):
    omit, sticky = dc.QUOTED[name]
    got = dc.finite_share(dc.want(name)), dc.finite_share(dc.want_sticky(name))
    print(name, got)
    assert np.allclose(got[0], omit, atol=6e-4, rtol=0), got[0]
    assert np.allclose(got[1], sticky, atol=6e-4, rtol=0), got[1]


def test_which_kinds_of_case_differ():
    """NaN in channel 0: from the first iteration.  One infinite pixel in channel 0: from the second.  Outside channel 0, or in every
    channel at the same pixel: never."""
    for case in dc.CASES.values():
        if not case.single:
            continue
        (_, _, c, v), = case.lace
        assert case.differs == (c == 0 and (v == "nan" or case.outer_iter >= 1)), case.name
    D = dc.CASES
    assert all(D["12x70x3-nan_at_3_10_0_and_pinf_at_8_50_2-iter%d" % k].differs for k in (0, 1))
    assert all(D["12x70x3-pinf_at_5_40_0_and_6_40_0-iter%d" % k].differs for k in (0, 1))
    assert all(D["12x70x3-pinf_at_5_40_0_and_7_40_0-iter%d" % k].differs for k in (0, 1))
    assert not any(D["12x70x3-nan_at_5_40_in_every_channel-iter%d" % k].differs for k in (0, 1))
    assert all(D["12x70x3-channel0_all_nan-iter%d" % k].differs for k in (0, 1, 5))


def test_adjacent_infinities_make_a_nan_inside_the_weights():
    """Inf - Inf: in the difference of two neighbours, and in Dver of the pixel between two infinite ones."""
    for name in ("12x70x3-pinf_at_5_40_0_and_6_40_0-iter0", "12x70x3-pinf_at_5_40_0_and_7_40_0-iter0"):
        I = dc.laced(name)
        assert not np.isnan(I).any()
        w = ref.diff_weights(I, channel_max=dc.sticky_max)
        assert any(np.isnan(x).any() for x in w), name
        assert all(np.isfinite(x).all() for x in ref.diff_weights(I)), name


# ---- the gateway cases ---------------------------------------------------------------------------------------------------------

def test_gateway_cases_cover_frames_shapes_and_eps():
    G = dc.GATES.values()
    assert {g.shape for g in G} == {(33, 29), (66, 258)} and {g.F for g in G} == {1, 2, 3, 4} and {g.eps for g in G} == {1e-3, 1e-5}
    assert {g.where for g in G if g.F >= 3} == {"first", "middle", "last", "every"}
    assert dc.gate_frames(3, "middle") == [1] and dc.gate_frames(4, "middle") == [2] and dc.gate_frames(4, "last") == [3]
    px = dc.GATE_PIXELS[(66, 258)]
    assert {(0, 0), (65, 257)} <= set(px) and {63, 64} <= {p[0] for p in px} and {63, 64, 255, 256} <= {p[1] for p in px}
    assert {(0, 0), (32, 28)} <= set(dc.GATE_PIXELS[(33, 29)])
    met = {}
    for g in G:  # every laced pixel meets NaN, +Inf and -Inf over the cases
        D = dc.gate_input(g.name)
        D3 = D if D.ndim == 3 else D[:, :, None]
        frames = dc.gate_frames(g.F, g.where)
        bad = np.zeros(D3.shape, bool)
        for i, j in dc.GATE_PIXELS[g.shape]:
            bad[i, j, frames] = True
            met.setdefault((g.shape, i, j), set()).add(float(D3[i, j, frames[0]]).__repr__())
        assert D.dtype == F32 and D3.shape == g.shape + (g.F,) and np.array_equal(~np.isfinite(D3), bad), g.name
    assert all(v == {"nan", "inf", "-inf"} for v in met.values()), met


@pytest.mark.parametrize("name", dc.GATE_NAMES)
def test_oracle_keeps_the_gateways_rule_at_nan(oracle, name):
    """oracle.DdiffWeights == the reference's compiled DdiffWeights == the numpy statement of the sticky rule, bit for bit with any NaN
    equal to any NaN.  A NaN of frame 0 stays, a NaN of a later frame is dropped: where the rules part, the case must show it."""
    _require_ref_build()
    g, D = dc.GATES[name], dc.gate_input(name)
    theirs = ref_lib.call("DdiffWeights", 4, D, F32(g.eps))
    ours = oracle.DdiffWeights(D, g.eps)
    stated = dc.gate_statement(D, g.eps)
    omit = dc.gate_statement(D, g.eps, channel_max=None)
    differ = keeps_nan = False
    for w, t, o, s, m in zip(("wW", "wN", "wE", "wS"), theirs, ours, stated, omit):
        assert t.shape == D.shape and o.shape == D.shape
        _eq(o, t, "%s %s: oracle against the compiled gateway" % (name, w))
        _eq(s, t, "%s %s: numpy statement against the compiled gateway" % (name, w))
        if D.ndim == 3:
            assert not t[:, :, 1:].any(), "%s: the gateway wrote frames above 0" % w
        differ |= not pb.bit_equal(s, m)
        keeps_nan |= bool(np.isnan(o).any())
        assert np.isfinite(m).all() == (g.where != "every"), w  # MATLAB's maximum would keep a NaN only where every frame has one
    # the case tells the rules apart exactly when NaN sits in frame 0 and not in every frame
    assert differ == (g.where == "first" and g.F > 1), name
    assert keeps_nan == (g.where in ("first", "every")), name
