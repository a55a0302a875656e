"""PDEIP_MODE_LINE_SCAN (line relaxation in the reference's line order, a line's two recurrences as scans): the cases, the
bounds and the runners that tests/test_line_scan_tolerance.py (reference side, no GPU) and tests/test_gpu_line_scan.py share.

The constants restate pdeip_alr.hpp (ALR_SCAN_*) and the decision of plan_alr (pdeip_alr_plan.hpp), as
seam_model.py restates the strip kernels': a lane of k_alr_scan holds VEC * G consecutive elements, G = 1, 2 or 3 chosen from the
line length and the number of coupled fields alone, 64 lanes scan by DPP in rows of 16, the wave totals cross the workgroup through
LDS; the two fields of a coupled model take half of the 1 024 threads each.
"""
from collections import namedtuple

import numpy as np

import problems as pb
import seam_model as sm

MODE_LINE_SCAN = 2
SCAN_VEC = 4                       # ALR_SCAN_VEC: elements of one group (one coef4)
SCAN_ROW = 16                      # lanes of one DPP row
SCAN_LANES = 64                    # ALR_SCAN_LANES
SCAN_THREADS = 1024                # ALR_SCAN_THREADS
SCAN_MAXG = 3                      # ALR_SCAN_MAXG
LEX_LDS_BYTES = 160 * 1024         # k_alr_lex's line buffers: the scan runs where they would hold every chain of the call

RMS_BOUND = 1e-4                   # the project's figure (BASELINE.json north_star), every case
TIGHT_OMEGA = 1.5                  # up to this relaxation factor additionally:
TIGHT_RMS, TIGHT_MAXABS = 1e-5, 1e-4
NOISE_ULP = 32                     # the reference's own response to +-32 ulp on its iterates must stay within a tenth of the bounds


def scan_groups(model, n):
    """G of the kernel that takes lines of n elements: the fields of a coupled model share the workgroup's threads."""
    return max(1, -(-n // (SCAN_THREADS // sm.ALR[model][0] * SCAN_VEC)))


def scan_runs(model, nrows, ncols):
    """Does a LINE_SCAN call of this frame run k_alr_scan, or k_alr_lex in both directions (plan_alr decides per call)?"""
    return sm.ALR[model][0] * 16 * max(nrows, ncols) <= LEX_LDS_BYTES


def scan_launches(model, nrows, ncols, it):
    """pdeip_last_launch_count() of a call that scans in both directions: the coefficient planes transposed (one launch per 16),
    the factor planes of both directions (2), then per iteration one pass along the columns -- every chain in it --, the iterate
    transposed, one pass along the rows, the iterate transposed back."""
    _, ntr, _ = sm.ALR[model]
    if model == "pde8":
        it = 1
    return 0 if it <= 0 else -(-ntr // sm.ALR_TB_MAX) + 2 + 4 * it


# ---- shapes -------------------------------------------------------------------------------------------------------------
BASE_SHAPES = [(3, 3), (2, 5), (5, 2), (5, 300), (260, 7), (97, 131), (131, 70), (1025, 6), (6, 1025), (2049, 5), (5, 2049)]
# one element to either side of every boundary of the scan tree, as column length and as row length
_SEAMS = sorted({b + d for b in (SCAN_VEC, 2 * SCAN_VEC, SCAN_ROW * SCAN_VEC, SCAN_LANES * SCAN_VEC, 2 * SCAN_LANES * SCAN_VEC,
                                 SCAN_THREADS // 2 * SCAN_VEC, SCAN_THREADS * SCAN_VEC) for d in (-1, 0, 1)})
_SEAMS_SINGLE = sorted({b + d for b in (LEX_LDS_BYTES // 32, 2 * SCAN_THREADS * SCAN_VEC) for d in (-1, 0, 1)})  # 5120: the coupled limit; 8192: G 2 -> 3
SEAM_LENGTHS = [n for n in _SEAMS if n >= 3]
SEAM_LENGTHS_SINGLE = _SEAMS_SINGLE
# the library takes frames of at least 3 x 3 (check_dims, every entry point and every mode); smaller ones are refused
REFUSED_SHAPES = [s for s in BASE_SHAPES if min(s) < 3]

Case = namedtuple("Case", "model nrows ncols nframes omega iters nan")

MODELS = {
    #          gateway                iterate planes  omega          nan plane(s)
    "elin4": ("Oflow_sor_elin4_2d", ("U", "V"), ("Cu", "Cv")),
    "llin4": ("Oflow_sor_llin4_2d", ("dU", "dV"), ("Cu", "Cv")),
    "llin8": ("Oflow_sor_llin8_2d", ("dU", "dV"), ("Cu", "Cv")),
    "disp4": ("Disp_sor_llin4_2d", ("dU",), ("Cu",)),
    "pde4": ("PDEsolver4", ("X",), ("TRACE",)),
    "pde8": ("PDEsolver8", ("X",), ("TRACE",)),
}
OMEGA = {"elin4": 1.5, "llin4": 1.4, "llin8": 1.4, "disp4": 1.4, "pde4": 1.3, "pde8": 1.3}
NAN_FRAC = 0.05


def _cases():
    out = []
    for shape in BASE_SHAPES:
        if shape in REFUSED_SHAPES:
            continue
        for model in MODELS:
            for F in ((1, 3) if model in ("pde4", "pde8") else (1,)):
                out.append(Case(model, shape[0], shape[1], F, OMEGA[model], (1, 3), True))
        out.append(Case("elin4", shape[0], shape[1], 1, 1.9, (4,), True))
    # the seams of the tree: a coupled model, a single-field model whose south row divides, a multi-frame model.  disp4 with one
    # iteration: on frames of 15 to 35 pixels its third iterate is large enough that +-32 ulp of it alone are 1.05e-6 to 1.11e-6 RMS,
    # past a tenth of the bound (test_line_scan_tolerance.py), and one iteration passes every seam in both directions
    for n in SEAM_LENGTHS:
        for model, F in (("elin4", 1), ("disp4", 1), ("pde4", 2)):
            for shape in sorted({(n, 5), (5, n)}):
                if shape not in BASE_SHAPES:
                    out.append(Case(model, shape[0], shape[1], F, OMEGA[model], (1,) if model == "disp4" else (1, 3), True))
    for n in SEAM_LENGTHS_SINGLE:
        for model, F in (("disp4", 1), ("pde4", 2)):
            for shape in ((n, 5), (5, n)):
                out.append(Case(model, shape[0], shape[1], F, OMEGA[model], (1,), True))
    out.append(Case("elin4", SCAN_LANES * SCAN_VEC + 1, SCAN_THREADS * SCAN_VEC - 1, 1, 1.5, (1,), True))  # both directions past one wave
    return out


CASES = _cases()
# BASELINE config C1's frame: RMS bound only (omega above TIGHT_OMEGA).  At the H&S driver's iter = 20 the reference's own response to
# +-32 ulp is 1.13e-5 RMS (max 1.1e-3), above a tenth of the 1e-4 bound, so that case is in neither list (test_line_scan_tolerance.py);
# iter = 4, the size test_alr_c1_size_exact_and_zebra runs, responds with 1.3e-6.
C1_CASE = Case("elin4", 388, 584, 1, 1.9, (4,), False)


def case_id(c):
    return "%s-%dx%dx%d-w%g-it%s%s" % (c.model, c.nrows, c.ncols, c.nframes, c.omega, "_".join(str(i) for i in c.iters), "-nan" if c.nan else "")


def bounds(c):
    """(rms, max-abs or None) a LINE_SCAN output plane of the case may differ from EXACT_ORDER's by."""
    if c.omega <= TIGHT_OMEGA:
        return TIGHT_RMS, TIGHT_MAXABS
    return RMS_BOUND, None


def problem(c):
    """The case's inputs: tests/problems.py draws (diagonally dominant: weights in [0.5, 5], data terms >= 0.05), then NaN at
    NAN_FRAC of the pixels of the data-term plane(s) alone -- `C` / TRACE, which Model::coef handles."""
    seed = 7000 + (c.nrows * 31 + c.ncols * 17 + c.nframes) % 997
    make = getattr(pb, c.model)
    p = make(seed, c.nrows, c.ncols) if c.model == "disp4" else make(seed, c.nrows, c.ncols, c.nframes)
    if c.model == "disp4":
        # problems.disp4 draws the base disparity in [-3, 3] and the solution follows it; the absolute bounds above were derived on
        # iterates of unit scale (32 ulp of 3 are 7.6e-6 on their own), so the base field is brought to the flow models' [-1, 1]
        p["U"] = np.asfortranarray(p["U"] / np.float32(3))
    if c.nan:
        rng = np.random.default_rng([seed, 0x6e616e])
        for name in MODELS[c.model][2]:
            p[name][rng.uniform(size=p[name].shape) < NAN_FRAC] = np.nan
    return p


def as_tuple(out):
    return out if isinstance(out, tuple) else (out,)


def run_oracle(oracle, c, p, it):
    """The reference's line order (order = 0), solver 2, through the gateway semantics of tests/oracle_lib.py."""
    return as_tuple(getattr(oracle, MODELS[c.model][0])(*p.values(), it, c.omega, solver=2, order=0))[:len(MODELS[c.model][1])]


def run_product(mex_api, c, p, it, solver=2):
    out = getattr(mex_api, MODELS[c.model][0])(*p.values(), np.float32(it), np.float32(c.omega), np.float32(solver))
    return as_tuple(out)[:len(MODELS[c.model][1])]


def differences(got, want):
    """[(rms, max-abs)] per output plane, in float64; NaN must sit at the same pixels."""
    out = []
    for g, w in zip(got, want):
        g, w = np.asarray(g, dtype=np.float64), np.asarray(w, dtype=np.float64)
        assert g.shape == w.shape
        assert np.array_equal(np.isnan(g), np.isnan(w)), "NaN at different pixels"
        d = np.nan_to_num(g - w, nan=0.0)
        out.append((float(np.sqrt(np.mean(d * d))), float(np.max(np.abs(d)))))
    return out


def disturb(rng, a, ulps=NOISE_ULP):
    """a moved by up to +-ulps units in the last place, uniformly drawn per element."""
    a = np.asarray(a, dtype=np.float32)
    s = rng.uniform(-1.0, 1.0, size=a.shape).astype(np.float32)
    with np.errstate(invalid="ignore"):
        return np.asfortranarray((a + s * np.float32(ulps) * np.spacing(np.abs(a))).astype(np.float32))


def disturbed_reference(oracle, c, it, seed=99):
    """-> (undisturbed, disturbed): the oracle run one iteration at a time, the second run with every iterate plane moved by
    +-NOISE_ULP ulp after each iteration."""
    rng = np.random.default_rng(seed)
    p = problem(c)
    names = MODELS[c.model][1]
    clean, noisy = dict(p), dict(p)
    steps = 1 if c.model == "pde8" else it  # the 9-point line solver runs one iteration whatever `iter` says
    for _ in range(steps):
        for name, plane in zip(names, run_oracle(oracle, c, clean, 1)):
            clean[name] = plane
        for name, plane in zip(names, run_oracle(oracle, c, noisy, 1)):
            noisy[name] = disturb(rng, plane)
    return tuple(clean[n] for n in names), tuple(noisy[n] for n in names)


# ---- the scan itself, in numpy float32 (what the CPU test holds against the serial Thomas solve) ----------------------------
def thomas_serial(a, b, c, d):
    """float32 Thomas solve in the reference's statement order (reciprocal of the denominator for the middle elements)."""
    f = np.float32
    n = len(b)
    cp, dp = np.zeros(n, f), np.zeros(n, f)
    cp[0], dp[0] = c[0] / b[0], d[0] / b[0]
    for k in range(1, n - 1):
        div = f(1.0) / (b[k] - cp[k - 1] * a[k])
        cp[k] = c[k] * div
        dp[k] = (d[k] - dp[k - 1] * a[k]) * div
    x = np.zeros(n, f)
    x[n - 1] = (d[n - 1] - dp[n - 2] * a[n - 1]) / (b[n - 1] - cp[n - 2] * a[n - 1])
    for k in range(n - 2, -1, -1):
        x[k] = dp[k] - cp[k] * x[k + 1]
    return x


def _scan_affine(m, t, chunk):
    """y[k] = m[k] y[k-1] + t[k], y[-1] = 0, in float32: chunks composed serially, Hillis-Steele across chunks, local fix-up."""
    f = np.float32
    n = len(m)
    nc = -(-n // chunk)
    M, T = np.ones(nc * chunk, f), np.zeros(nc * chunk, f)
    M[:n], T[:n] = m, t
    M, T = M.reshape(nc, chunk), T.reshape(nc, chunk)
    sm_, st_ = np.ones(nc, f), np.zeros(nc, f)
    for e in range(chunk):
        st_ = (M[:, e] * st_ + T[:, e]).astype(f)
        sm_ = (M[:, e] * sm_).astype(f)
    step = 1
    while step < nc:  # inclusive scan of the chunk maps
        pm, pt = np.ones(nc, f), np.zeros(nc, f)
        pm[step:], pt[step:] = sm_[:-step], st_[:-step]
        st_ = (sm_ * pt + st_).astype(f)
        sm_ = (sm_ * pm).astype(f)
        step *= 2
    y = np.zeros(nc, f)
    y[1:] = st_[:-1]  # entering value of every chunk: the inclusive map of the chunks before it applied to 0
    out = np.zeros((nc, chunk), f)
    for e in range(chunk):
        y = (M[:, e] * y + T[:, e]).astype(f)
        out[:, e] = y
    return out.reshape(-1)[:n]


def thomas_scan(a, b, c, d, chunk=2 * SCAN_VEC):
    """The same solve with both recurrences as chunked scans; cp and the divisors serially, as alr_factor builds them."""
    f = np.float32
    n = len(b)
    cp, rec = np.zeros(n, f), np.zeros(n, f)
    cp[0], rec[0] = c[0] / b[0], f(1.0) / b[0]
    for k in range(1, n - 1):
        rec[k] = f(1.0) / (b[k] - cp[k - 1] * a[k])
        cp[k] = c[k] * rec[k]
    rec[n - 1] = f(1.0) / (b[n - 1] - cp[n - 2] * a[n - 1])
    dp = _scan_affine((-(a * rec)).astype(f), (d * rec).astype(f), chunk)
    x = _scan_affine((-cp[::-1]).astype(f), dp[::-1].astype(f), chunk)
    return x[::-1]
