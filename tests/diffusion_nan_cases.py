"""The inputs of tests/test_gpu_diffusion_nan.py: images and frame stacks with NaN, +Inf or -Inf laced in, each chosen for the one
place where the two users of k_diffweights6 (csrc/pdeip_pointwise.hpp) must part.  tests/test_diffusion_nan_cases.py proves on the
CPU that every case is what it claims; without that a case could pass while testing nothing.

The maximum over the channels (frames) has two contracts:
    omit    Diffusion4_v10.m's DiffWeights takes max(w, [], 3), which omits a NaN of ANY channel: np.fmax.reduce (diffusion_ref.py).
    sticky  the C gateway DdiffWeights (imageDiffusionWeights.c, Calc_wW :143 and its siblings) starts from frame 0 and lets a later
            frame replace it when t > m: a NaN of frame 0 stays, a NaN of a later frame is dropped (sticky_max below).
They agree on finite terms, on +Inf (it wins either way) and on a NaN outside channel 0, or in every channel at once.  They part where
a term of channel 0 is NaN and another channel's is not.  A NaN pixel of channel 0 does that in the first iteration; a single +-Inf
pixel only in the second, when the first has turned its row and column into NaN (0 * Inf in the Thomas solve: the weights beside an
infinite gradient are 1/sqrt(Inf) = 0); two +Inf pixels side by side, or with one pixel between them, give Inf - Inf at once.
Each diffusion case carries that claim as `differs`.

Positions: the interior, pixel (0, 0), the last pixel, and both sides of rows 63|64 and 255|256 and of columns 63|64 -- the ends of
the line kernel's 64-lane blocks and of the weight kernel's 256-row blocks.  Arrays are MATLAB-shaped float32 [rows, cols(, F)],
built once per process and read-only; references are computed once per process and shared.
"""
import collections
import functools

import numpy as np

import diffusion_ref as ref
import problems as pb

F32 = np.float32
VALUES = {"nan": np.nan, "pinf": np.inf, "ninf": -np.inf}


def _ro(a):
    a = np.asfortranarray(a, dtype=F32)
    a.setflags(write=False)
    return a


def sticky_max(T):
    """The gateway's maximum over the last axis: frame 0 initialises, a later frame replaces it when t > m."""
    m = T[..., 0]
    for k in range(1, T.shape[-1]):
        t = T[..., k]
        with np.errstate(invalid="ignore"):
            m = np.where(t > m, t, m)
    return m


def finite_share(a):
    """Per channel (frame) of [rows, cols, C]."""
    return [float(np.isfinite(a[:, :, k]).mean()) for k in range(a.shape[2])]


# ---- Diffusion4_v10 ------------------------------------------------------------------------------------------------------------

def image(shape):
    """Piecewise-smooth 0..255 content as test_gpu_diffusion._image draws it: blocks of constant grey with noise."""
    rng = np.random.default_rng(500 + 7 * shape[0] + shape[1] + shape[2])
    blocks = rng.uniform(0, 255, (max(1, shape[0] // 16) + 1, max(1, shape[1] // 16) + 1) + tuple(shape[2:]))
    I = blocks[np.arange(shape[0]) // 16][:, np.arange(shape[1]) // 16] + rng.normal(0, 6, shape)
    return np.clip(I, 0, 255).astype(F32)


# name: the case's id.  lace: ((i, j, c, value key), ...), None for a whole axis.  single: one pixel of one channel.
# differs: the omit rule and the sticky rule give different outputs (see the module's docstring).
Case = collections.namedtuple("Case", "name shape lace outer_iter single differs")

# (shape, interior pixel, ((pixel, the infinity laced there), ...)): every value in every channel at the interior pixel; elsewhere NaN
# in channel 0 and in the last channel, the named infinity in channel 0 and the other one in a middle channel
LAYOUT = (
    ((12, 70, 3), (5, 40), (((0, 0), "pinf"), ((11, 69), "ninf"), ((5, 63), "pinf"), ((5, 64), "ninf"))),
    ((66, 9, 2), (30, 4), (((0, 0), "ninf"), ((65, 8), "pinf"), ((63, 4), "ninf"), ((64, 4), "pinf"))),
    ((258, 66, 4), (100, 30), (((0, 0), "pinf"), ((257, 65), "ninf"), ((63, 30), "pinf"), ((64, 30), "ninf"), ((255, 30), "pinf"),
                               ((256, 30), "ninf"), ((100, 63), "pinf"), ((100, 64), "ninf"), ((255, 63), "pinf"), ((256, 64), "ninf"))),
    ((3, 3, 3), (1, 1), ()),
    ((2, 2, 2), (0, 0), ()),
)
A = LAYOUT[0][0]


def _sid(shape):
    return "x".join(map(str, shape))


def claim_differs(shape, lace, outer_iter):
    """The module docstring's reasoning as a rule, from the laced pixels alone (nothing is computed)."""
    bad = {}
    for i, j, c, v in lace:
        bad.setdefault((i, j), {})[c] = v
    ch0 = {p: cv[0] for p, cv in bad.items() if 0 in cv and len(cv) < shape[2]}  # channel 0 laced, and not every channel with it
    if not ch0:
        return False
    if any(v == "nan" for v in ch0.values()) or ref.iterations(outer_iter) >= 2:
        return True
    inf = sorted(p for p in ch0 if None not in p)  # Inf - Inf between two infinite pixels one or two apart on a line
    return any(a != b and ((a[0] == b[0] and abs(a[1] - b[1]) <= 2) or (a[1] == b[1] and abs(a[0] - b[0]) <= 2)) for a in inf for b in inf)


def _cases():
    T = collections.OrderedDict()

    def add(shape, lace, outer_iter, what, single=False):
        name = "%s-%s-iter%g" % (_sid(shape), what, outer_iter)
        assert name not in T, name
        T[name] = Case(name, shape, tuple(lace), outer_iter, single, claim_differs(shape, lace, outer_iter))

    def one(shape, p, c, v):
        for outer_iter in (0, 1):
            add(shape, [(p[0], p[1], c, v)], outer_iter, "%s_at_%d_%d_%d" % (v, p[0], p[1], c), single=True)

    for shape, interior, others in LAYOUT:
        C = shape[2]
        for v in VALUES:
            for c in range(C):
                one(shape, interior, c, v)
        for p, inf in others:
            one(shape, p, 0, "nan")
            one(shape, p, C - 1, "nan")
            one(shape, p, 0, inf)
            if C > 2:
                one(shape, p, C // 2, "ninf" if inf == "pinf" else "pinf")
    for outer_iter in (0, 1):
        add(A, [(3, 10, 0, "nan"), (8, 50, 2, "pinf")], outer_iter, "nan_at_3_10_0_and_pinf_at_8_50_2")
        add(A, [(5, 40, 0, "pinf"), (6, 40, 0, "pinf")], outer_iter, "pinf_at_5_40_0_and_6_40_0")  # Inf - Inf in the difference
        add(A, [(5, 40, 0, "pinf"), (7, 40, 0, "pinf")], outer_iter, "pinf_at_5_40_0_and_7_40_0")  # Inf - Inf inside Dver at (6, 40)
        add(A, [(5, 40, c, "nan") for c in range(3)], outer_iter, "nan_at_5_40_in_every_channel")
    for outer_iter in (0, 1, 5):
        add(A, [(None, None, 0, "nan")], outer_iter, "channel0_all_nan")
    return T


CASES = _cases()
NAMES = tuple(CASES)
SINGLE = tuple(n for n in NAMES if CASES[n].single)
FLOOD = "12x70x3-nan_at_5_40_in_every_channel-iter1"  # the one case whose output is NaN everywhere, under both rules
# the finite share per channel of the outputs by which these cases were chosen: (omit rule, sticky rule), to three decimals
QUOTED = {
    "12x70x3-nan_at_5_40_0-iter0": ([0.904, 1, 1], [0.718] * 3),
    "12x70x3-nan_at_5_40_0-iter1": ([0, 1, 1], [0] * 3),
    "12x70x3-pinf_at_5_40_0-iter1": ([0, 1, 1], [0] * 3),
    "66x9x2-nan_at_65_8_0-iter0": ([0.875, 1], [0.754] * 2),
    "258x66x4-nan_at_255_63_0-iter0": ([0.981, 1, 1, 1], [0.943] * 4),
    "258x66x4-ninf_at_256_64_0-iter1": ([0, 1, 1, 1], [0] * 4),
    "12x70x3-channel0_all_nan-iter0": ([0, 1, 1], [0] * 3),
    "12x70x3-channel0_all_nan-iter1": ([0, 1, 1], [0] * 3),
    "12x70x3-channel0_all_nan-iter5": ([0, 1, 1], [0] * 3),
    "3x3x3-nan_at_1_1_0-iter0": ([0.444, 1, 1], [0] * 3),
    "2x2x2-nan_at_0_0_0-iter0": ([0.25, 1], [0] * 2),
}


@functools.lru_cache(maxsize=None)
def laced(name):
    """The case's image [rows, cols, C]."""
    case = CASES[name]
    I = image(case.shape)
    for i, j, c, v in case.lace:
        I[slice(None) if i is None else i, slice(None) if j is None else j, c] = F32(VALUES[v])
    return _ro(I)


def touched(case):
    """The channels a case laces."""
    return sorted({c for _, _, c, _ in case.lace})


@functools.lru_cache(maxsize=None)
def want(name):
    """diffusion_ref.Diffusion4_v10 of the case with the default alpha: the .m's rule, what pdeip_diffusion4 must give."""
    return _ro(ref.Diffusion4_v10(laced(name), outer_iter=CASES[name].outer_iter))


@functools.lru_cache(maxsize=None)
def want_sticky(name):
    """The same iterations with the gateway's maximum in place of the .m's: what the driver gave while it used the gateway's kernel
    as it stood."""
    return _ro(ref.Diffusion4_v10(laced(name), outer_iter=CASES[name].outer_iter, channel_max=sticky_max))


# ---- the DdiffWeights gateway --------------------------------------------------------------------------------------------------

# shape -> the laced pixels: corners, the interior, and both sides of rows 63|64 and of columns 63|64 and 255|256
GATE_PIXELS = {
    (33, 29): ((0, 0), (32, 28), (16, 14), (0, 28), (32, 0), (10, 20)),
    (66, 258): ((0, 0), (65, 257), (30, 100), (63, 5), (64, 12), (20, 63), (25, 64), (40, 255), (45, 256), (63, 63), (64, 64)),
}
GATE_EPS = (1e-3, 1e-5)
Gate = collections.namedtuple("Gate", "name shape F where eps")


def gate_frames(F, where):
    """The frames a case laces: frame 0 only, a middle frame only, the last frame only, or every frame."""
    return {"first": [0], "middle": [F // 2], "last": [F - 1], "every": list(range(F))}[where]


def _gates():
    T = collections.OrderedDict()
    for shape in GATE_PIXELS:
        for F in (1, 2, 3, 4):
            # one frame: the first, the last and every frame are the same one; two frames: no frame between them
            for where in (("every",) if F == 1 else ("first", "last", "every") if F == 2 else ("first", "middle", "last", "every")):
                for eps in GATE_EPS:
                    name = "%s_F%d-%s-eps%g" % (_sid(shape), F, where, eps)
                    T[name] = Gate(name, shape, F, where, eps)
    return T


GATES = _gates()
GATE_NAMES = tuple(GATES)


@functools.lru_cache(maxsize=None)
def gate_input(name):
    """D [rows, cols(, F)]: the values of problems.diffweights with NaN, +Inf and -Inf taking turns over the laced pixels; the turn
    starts at a value that depends on the case, so that every pixel meets every value over the cases."""
    g = GATES[name]
    D = pb.diffweights(600 + g.shape[0] + g.F, g.shape[0], g.shape[1], g.F)["D"].copy(order="F")
    keys = list(VALUES)
    turn = g.F + ["first", "middle", "last", "every"].index(g.where)
    for n, (i, j) in enumerate(GATE_PIXELS[g.shape]):
        for k in gate_frames(g.F, g.where):
            D[(i, j, k) if g.F > 1 else (i, j)] = F32(VALUES[keys[(n + turn) % 3]])
    return _ro(D)


def gate_statement(D, eps, channel_max=sticky_max):
    """[wW, wN, wE, wS] of the gateway in numpy, in D's shape: frame 0 holds the weights of the sticky maximum, the frames above it
    stay zero (DdiffWeights.c writes frame 0 only)."""
    outs = []
    for w in ref.diff_weights(D, channel_max=channel_max, eps=eps):
        o = np.zeros(D.shape, F32, order="F")
        o[(slice(None), slice(None), 0) if D.ndim == 3 else Ellipsis] = w
        outs.append(o)
    return outs
