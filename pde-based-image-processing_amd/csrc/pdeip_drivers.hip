// pdeip_drivers.hip -- libpdeip.so: the eight drivers runme.m calls, as host-pointer entry points that keep a whole coarse-to-fine
// run resident on the device.
//
//   [U V] = FlowEminND_llin_2D_v10(Iin, channels, fstTerm, sndTerm, ...)   matlab/optical_flow/FlowEminND_llin_2D_v10.m:52-369       pdeip_flow_nd_llin
//   [U V] = FlowEminAD_llin_2D_v10(...)                                     matlab/optical_flow/FlowEminAD_llin_2D_v10.m:52-383       pdeip_flow_ad_llin
//   [U V] = FlowEminHS_elin_2D_v10(Iin, channels, ...)                      matlab/optical_flow/FlowEminHS_elin_2D_v10.m:52-200       pdeip_flow_hs_elin
//   [U V] = FlowEminNDFASFMG_elin_2D_v10(Iin, channels, ...)                matlab/optical_flow/FlowEminNDFASFMG_elin_2D_v10.m:53-273 pdeip_flow_fas_fmg_elin
//   U     = DispEminND_llin_2D(Il, Ir, fstTerm, sndTerm, ...)              matlab/disparity/DispEminND_llin_2D.m:51-316              pdeip_disp_nd_llin
//   U     = DispEminND_llin_sym_2D(Il, Ir, ...)                            matlab/disparity/DispEminND_llin_sym_2D.m:51-275          pdeip_disp_nd_llin_sym
//   Iout  = TVdenoise8(I_in, ...) / TVdenoise4(I_in, ...)                  matlab/denoising/TVdenoise{8,4}.m                         pdeip_tvdenoise8 / 4
//
// A MATLAB session that only swaps the MEX gateways pays 13-17 planes of PCIe traffic per solver call (7.8 ms per 4K call,
// INTEGRATION.md); calling these instead moves the frames up once and the result down once.  The level loops below are host
// control flow around the library's own device entry points -- the same `_dev` stage kernels, in the same order and with
// the same arguments, as the Python drivers (drivers.py / flow_level.py / fas.py / pyramid.py), which the tests compare with bit
// for bit.  The pyramid's imresize / imfilter / fspecial are the definitions of pyramid.py (csrc/pdeip_pyr.hpp), there
// being no Image Processing Toolbox to compare with.  Ordering and solver as everywhere: pdeip_set_mode / PDEIP_MODE,
// param.solver.
//
// What the drivers have in common is stated once, in this order:
//   Run, play()                     one run's stream and device arena; every driver is played twice, dry for its size, then for real
//   upload_frames, zero_plane,      the ends of every run: frames up, a zero start field, results down
//   download
//   or_default, merge()             "<= 0 or NaN is the driver's default", and the four parameter structs as field lists
//   solve_*                         SOR or line relaxation from param.solver, one helper per model
//   build_pyramid, PyramidRule      the image pyramid; what differs between the drivers is the rule they pass
//   DataTerms                       the warped frames and their derivatives of the three late-linearisation levels
//   llin_driver                     the scale loop of pdeip_flow_nd_llin, pdeip_flow_ad_llin and pdeip_disp_nd_llin, over one or two fields
//   enter()                         what every entry point refuses before it touches the device, and in which order
// and the drivers themselves are what is left: their levels (flow_level, flow_ad_level, disp_level, sym_level, Fas), the four
// scale loops that are not the late-linearisation one (disp_sym, flow_hs, flow_tvl1, fas_fmg, tv_run) and the entry points.
#include "pdeip_ctx.hpp"

#include <cmath>
#include <initializer_list>
#include <utility>
#include <vector>

using namespace pdeip;

namespace {

constexpr int ALL_SCALES = 0x7fffffff; // param.scales not given: the pyramid ends where the frame is small enough

__global__ void k_scale(float *out, const float *in, size_t n, float s, int divide)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = divide ? in[i] / s : in[i] * s; // a true division where MATLAB divides (Iin ./ 255)
}

__global__ void k_fill(float *out, size_t n, float v)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = v;
}

// One run: a stream, a device arena and a dry mode.  The arena is one cached workspace buffer per device, bump-allocated;
// a run is played twice -- dry (nothing is launched: the sizes only depend on the frame's dimensions) to learn how much it
// needs, then for real.
struct Run {
    hipStream_t s = nullptr;
    bool dry = true;
    int rc = PDEIP_OK, mode = PDEIP_MODE_EXACT_ORDER;
    char *base = nullptr;
    size_t used = 0, peak = 0;
    void *take(size_t bytes)
    {
        const size_t at = (used + 255) & ~(size_t)255;
        used = at + bytes;
        if (used > peak) peak = used;
        return base + at; // dry: base is null and nothing dereferences it
    }
    float *planes(int nrows, int ncols, int frames = 1) { return static_cast<float *>(take(sizeof(float) * (size_t)nrows * ncols * frames)); }
    double *dplane(int nrows, int ncols) { return static_cast<double *>(take(sizeof(double) * (size_t)nrows * ncols)); }
    size_t mark() const { return used; }
    void release(size_t m) { used = m; }
};
#define DO(R, expr)                                                \
    do {                                                           \
        if (!(R).dry && (R).rc == PDEIP_OK) (R).rc = (expr);       \
    } while (0)
#define DOHIP(R, expr)                                                                                                      \
    do {                                                                                                                    \
        if (!(R).dry && (R).rc == PDEIP_OK && (expr) != hipSuccess) (R).rc = set_err(PDEIP_ERR_DEVICE, "%s failed", #expr); \
    } while (0)

template <class Body> int play(const char *who, Body body)
{
    RC(use_device());
    Run plan;
    body(plan); // dry: sizes only
    float *arena = nullptr;
    RC(ws_get(WS_DRIVER, plan.peak + 256, &arena));
    Run R;
    R.dry = false;
    R.base = reinterpret_cast<char *>(arena);
    R.mode = g.mode;
    R.s = nullptr; // the host entry points use the device's default stream
    body(R);
    if (R.rc != PDEIP_OK) return R.rc;
    if (R.used > plan.peak + 256) return set_err(PDEIP_ERR_DEVICE, "%s: the run used more device memory than its plan", who);
    RC(pdeip_persist_error());
    return PDEIP_OK;
}

void scale(Run &R, float *out, const float *in, size_t n, float s, bool divide)
{
    if (R.dry || R.rc != PDEIP_OK) return;
    hipLaunchKernelGGL(k_scale, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, R.s, out, in, n, s, divide ? 1 : 0);
}

void fill(Run &R, float *out, size_t n, float v)
{
    if (R.dry || R.rc != PDEIP_OK) return;
    hipLaunchKernelGGL(k_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, R.s, out, n, v);
}

// Both frames of a run as [2C] planes on the device, from one host array that holds both (b null) or from one array each;
// div255: Iin = single(Iin) ./ 255 into a second set of planes.
float *upload_frames(Run &R, const float *a, const float *b, int nrows, int ncols, int C, bool div255)
{
    const size_t n = (size_t)nrows * ncols * C;
    float *up = R.planes(nrows, ncols, 2 * C), *fr = div255 ? R.planes(nrows, ncols, 2 * C) : up;
    if (b == nullptr) {
        DOHIP(R, hipMemcpyAsync(up, a, 2 * n * sizeof(float), hipMemcpyHostToDevice, R.s));
    } else {
        DOHIP(R, hipMemcpyAsync(up, a, n * sizeof(float), hipMemcpyHostToDevice, R.s));
        DOHIP(R, hipMemcpyAsync(up + n, b, n * sizeof(float), hipMemcpyHostToDevice, R.s));
    }
    if (div255) scale(R, fr, up, 2 * n, 255.0f, true);
    return fr;
}

float *zero_plane(Run &R, int nrows, int ncols) // "zero flow" at the coarsest scale
{
    float *p = R.planes(nrows, ncols);
    DOHIP(R, hipMemsetAsync(p, 0, (size_t)nrows * ncols * sizeof(float), R.s));
    return p;
}

// {host, device} arrays of n floats each down to the host (a null host pointer: the driver has no such result), then the run's one wait
void download(Run &R, std::initializer_list<std::pair<float *, const float *>> results, size_t n)
{
    for (const auto &r : results)
        if (r.first != nullptr) DOHIP(R, hipMemcpyAsync(r.first, r.second, n * sizeof(float), hipMemcpyDeviceToHost, R.s));
    DOHIP(R, hipStreamSynchronize(R.s));
}

// The parameter structs of include/pdeip.h: a field that is <= 0 or NaN means the driver's default.  This is the one statement of
// that rule; the four merges below are field lists.
double or_default(double v, double dflt) { return v > 0.0 ? v : dflt; }
int or_default(int v, int dflt) { return v > 0 ? v : dflt; }
#define TAKE(field) p.field = or_default(u->field, p.field)

struct Params { // pdeip_driver_params, defaults filled in
    double alpha, omega, gammaS, b1, b2, scl_factor;
    int firstLoop, secondLoop, iter, solver, scales;
};
Params merge(const pdeip_driver_params *u, Params p)
{
    if (u == nullptr) return p;
    TAKE(alpha), TAKE(omega), TAKE(gammaS), TAKE(b1), TAKE(b2), TAKE(scl_factor);
    TAKE(firstLoop), TAKE(secondLoop), TAKE(iter), TAKE(solver), TAKE(scales);
    return p;
}
struct SymParams {
    double alpha, beta, omega, b1, b2, scl_factor;
    int firstLoop, secondLoop, iter, solver;
};
SymParams merge(const pdeip_sym_params *u, SymParams p)
{
    if (u == nullptr) return p;
    TAKE(alpha), TAKE(beta), TAKE(omega), TAKE(b1), TAKE(b2), TAKE(scl_factor);
    TAKE(firstLoop), TAKE(secondLoop), TAKE(iter), TAKE(solver);
    return p;
}
struct FasParams {
    double alpha, omega, b1, b2, scl_factor;
    int firstLoop, iter, solver, cycle_index, scales;
};
FasParams merge(const pdeip_fas_params *u, FasParams p)
{
    if (u == nullptr) return p;
    TAKE(alpha), TAKE(omega), TAKE(b1), TAKE(b2), TAKE(scl_factor);
    TAKE(firstLoop), TAKE(iter), TAKE(solver), TAKE(cycle_index), TAKE(scales);
    return p;
}
struct TvParams {
    double alpha, omega, scl, scl_factor;
    int outer_iter, inner_iter, solver;
};
TvParams merge(const pdeip_tv_params *u, TvParams p)
{
    if (u == nullptr) return p;
    TAKE(alpha), TAKE(omega), TAKE(scl), TAKE(scl_factor);
    TAKE(outer_iter), TAKE(inner_iter), TAKE(solver);
    return p;
}
#undef TAKE

// param.solver: successive over-relaxation (in the ordering of the run's mode) or alternating line relaxation -- one dispatch per
// model, on the planes in the order of the solver's own argument list.
struct Solver {
    int which, iter; // param.solver; sweeps per call
    float omega;
    bool sor() const { return which == PDEIP_SOLVER_SOR; }
};
// c: MGd, CuGd, CvGd, DuGd, DvGd, wW, wN, wE, wS
void solve_elin4(Run &R, const Solver &v, float *U, float *V, float *const (&c)[9], int nr, int nc)
{
    if (v.sor()) DO(R, pdeip_oflow_sor_elin4_dev(R.s, U, V, c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], nr, nc, v.iter, v.omega, R.mode, 0));
    else DO(R, pdeip_oflow_alr_elin4_dev(R.s, U, V, c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], nr, nc, v.iter, v.omega, R.mode));
}
void solve_flow_llin4(Run &R, const Solver &v, float *U, float *V, float *dU, float *dV, float *const (&c)[9], int nr, int nc)
{
    if (v.sor()) DO(R, pdeip_oflow_sor_llin4_dev(R.s, U, V, dU, dV, c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], nr, nc, v.iter, v.omega, R.mode, 0));
    else DO(R, pdeip_oflow_alr_llin4_dev(R.s, U, V, dU, dV, c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], nr, nc, v.iter, v.omega, R.mode));
}
// Oflow_sor_llin8_2d: c: MGd .. DvGd; w: wW, wNW, wN, wNE, wE, wSE, wS, wSW.  Its point solver runs the 4-neighbour arithmetic on W, N,
// E, S (opticalflowSolvers.c:1487); line relaxation takes all eight.
void solve_flow_llin8_or_4(Run &R, const Solver &v, float *U, float *V, float *dU, float *dV, float *const (&c)[5], float *const (&w)[8], int nr, int nc)
{
    if (v.sor()) DO(R, pdeip_oflow_sor_llin4_dev(R.s, U, V, dU, dV, c[0], c[1], c[2], c[3], c[4], w[0], w[2], w[4], w[6], nr, nc, v.iter, v.omega, R.mode, 0));
    else DO(R, pdeip_oflow_alr_llin8_dev(R.s, U, V, dU, dV, c[0], c[1], c[2], c[3], c[4], w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], nr, nc, v.iter, v.omega, R.mode));
}
void solve_disp_llin4(Run &R, const Solver &v, float *U, float *dU, float *CuGd, float *DuGd, float *const (&w)[4], int nr, int nc) // w: wW, wN, wE, wS
{
    if (v.sor()) DO(R, pdeip_disp_sor_llin4_dev(R.s, U, dU, CuGd, DuGd, w[0], w[1], w[2], w[3], nr, nc, v.iter, v.omega, R.mode, 0));
    else DO(R, pdeip_disp_alr_llin4_dev(R.s, U, dU, CuGd, DuGd, w[0], w[1], w[2], w[3], nr, nc, v.iter, v.omega, R.mode));
}
void solve_pde4(Run &R, const Solver &v, float *X, float *TRACE, float *B, float *const (&w)[8], int nr, int nc, int F) // the first four of w
{
    if (v.sor()) DO(R, pdeip_pde_sor4_dev(R.s, X, TRACE, B, w[0], w[1], w[2], w[3], nr, nc, F, v.iter, v.omega, R.mode, 0));
    else DO(R, pdeip_pde_alr4_dev(R.s, X, TRACE, B, w[0], w[1], w[2], w[3], nr, nc, F, v.iter, v.omega, R.mode));
}
void solve_pde8(Run &R, const Solver &v, float *X, float *TRACE, float *B, float *const (&w)[8], int nr, int nc, int F)
{
    if (v.sor()) DO(R, pdeip_pde_sor8_dev(R.s, X, TRACE, B, w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], nr, nc, F, v.iter, v.omega, R.mode, 0));
    else DO(R, pdeip_pde_alr8_dev(R.s, X, TRACE, B, w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], nr, nc, F, v.iter, v.omega, R.mode));
}

// numpy.ndarray.sum() of a contiguous float64 array of n < 128 elements: eight running sums r[0..7] over i = 0, 8, 16, ... then
// ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the tail added one by one (numpy/core/src/umath/loops_utils.h.src,
// pairwise_sum).  The Gaussian mask is divided by this sum; pyramid.py (numpy) is the definition the tests compare with.
double numpy_sum(const std::vector<double> &a)
{
    const size_t n = a.size();
    if (n < 8) {
        double r = 0.0; // numpy: res = 0.; res += a[i] (with a -0.0 start that does not matter for positive terms)
        for (size_t i = 0; i < n; i++) r += a[i];
        return r;
    }
    double r[8];
    for (int k = 0; k < 8; k++) r[k] = a[k];
    size_t i = 8;
    for (; i + 8 <= n; i += 8)
        for (int k = 0; k < 8; k++) r[k] += a[i + k];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; i++) res += a[i];
    return res;
}

} // namespace

namespace pdeip {
// fspecial('gaussian', [size size], sigma) as pyramid.py states it: row-major doubles, divided by their numpy sum
std::vector<double> gaussian_mask(int size, double sigma)
{
    const int r = size / 2;
    std::vector<double> g((size_t)size * size);
    for (int a = -r; a <= r; a++)
        for (int b = -r; b <= r; b++) g[(size_t)(a + r) * size + (b + r)] = std::exp(-((double)(a * a) + (double)(b * b)) / (2.0 * sigma * sigma));
    const double s = numpy_sum(g);
    for (double &v : g) v /= s;
    return g;
}
} // namespace pdeip

namespace {

// imresize(A, [out_rows out_cols], 'bilinear') of a DOUBLE array on the host, as pyramid.resize(..., out_dtype=float64) does it:
// triangle kernel at MATLAB's pixel-centre convention, stretched by 1/scale when shrinking, taps normalised, rows first, then
// columns, every sum left to right.  A: column-major [nrows x ncols].  (The a-priori fields only: a few small planes per run.)
struct Taps {
    int T = 0;
    std::vector<int> idx;   // [n_out][T], clamped
    std::vector<double> w;  // [n_out][T], normalised
};
Taps resize_taps(int n_in, int n_out)
{
    Taps t;
    const double scale = (double)n_out / (double)n_in;
    const double stretch = scale >= 1.0 ? 1.0 : 1.0 / scale;
    const double width = 1.0 * stretch;
    t.T = (int)std::ceil(2.0 * width) + 2;
    t.idx.resize((size_t)n_out * t.T);
    t.w.resize((size_t)n_out * t.T);
    for (int o = 0; o < n_out; o++) {
        const double x = ((double)o + 0.5) / scale - 0.5;
        const long first = (long)std::floor(x - width);
        double total = 0.0;
        for (int k = 0; k < t.T; k++) {
            const long id = first + k;
            const double a = std::fabs(((double)id - x) / stretch);
            const double wk = (1.0 - a) > 0.0 ? (1.0 - a) : 0.0;
            t.w[(size_t)o * t.T + k] = wk;
            total = k == 0 ? wk : total + wk;
            t.idx[(size_t)o * t.T + k] = (int)(id < 0 ? 0 : (id > n_in - 1 ? n_in - 1 : id));
        }
        for (int k = 0; k < t.T; k++) t.w[(size_t)o * t.T + k] /= total;
    }
    return t;
}
std::vector<double> resize_double(const std::vector<double> &A, int nrows, int ncols, int out_rows, int out_cols)
{
    const Taps r = resize_taps(nrows, out_rows), c = resize_taps(ncols, out_cols);
    std::vector<double> T1((size_t)out_rows * ncols), out((size_t)out_rows * out_cols);
    for (int j = 0; j < ncols; j++)
        for (int o = 0; o < out_rows; o++) {
            double acc = r.w[(size_t)o * r.T] * A[(size_t)j * nrows + r.idx[(size_t)o * r.T]];
            for (int k = 1; k < r.T; k++) acc = acc + r.w[(size_t)o * r.T + k] * A[(size_t)j * nrows + r.idx[(size_t)o * r.T + k]];
            T1[(size_t)j * out_rows + o] = acc;
        }
    for (int o2 = 0; o2 < out_cols; o2++)
        for (int o = 0; o < out_rows; o++) {
            double acc = c.w[(size_t)o2 * c.T] * T1[(size_t)c.idx[(size_t)o2 * c.T] * out_rows + o];
            for (int k = 1; k < c.T; k++) acc = acc + c.w[(size_t)o2 * c.T + k] * T1[(size_t)c.idx[(size_t)o2 * c.T + k] * out_rows + o];
            out[(size_t)o2 * out_rows + o] = acc;
        }
    return out;
}

struct Level {
    int nr = 0, nc = 0;
    float *I0 = nullptr, *I1 = nullptr; // [C] planes each; a pyramid of one image has no I1
    double *Us = nullptr, *Vs = nullptr; // the a-priori fields of the scale on the device (or null)
    size_t n() const { return (size_t)nr * nc; }
};

// The image pyramid (FlowEminND_llin_2D_v10.m:100-127 / DispEminND_llin_2D.m:77-104 / TVdenoise8.m:52-72): resize to
// ceil(size * scl_factor), the level just left is smoothed after it has been resized.  What the drivers do differently is the rule:
struct PyramidRule {
    double scl_factor;
    int max_scales;           // param.scales: the loop `for scl=2:param.scales` simply ends, the last scale as resized
    int stop_rows, stop_cols; // the scale that is this small is the last one ...
    bool smooth_last;         // ... and is smoothed too -- or left as resized: DispEminND_llin_sym_2D.m:94-98, and TVdenoise8.m:72, which
                              // writes the smoothed scale to a misspelt variable
    int gsize;                // fspecial('gaussian', [gsize gsize], sigma)
    double sigma;
    bool stop_when_stuck;     // a scale that no longer shrinks (ceil(n * scl_factor) == n both ways) is the last one as well.  The TV
                              // drivers only, which have no param.scales: the reference's loop would not end.  The others go on to
                              // param.scales with scales of one size, as pyramid.build_dev does.
};
std::vector<Level> build_pyramid(Run &R, int images, float *f0, float *f1, int nrows, int ncols, int C, const PyramidRule &q)
{
    const std::vector<double> G = gaussian_mask(q.gsize, q.sigma);
    // per image of the pyramid (a dry run's planes are offsets from a null base: no pointer says whether there is a second image)
    auto resized = [&](const Level &from, Level &to) {
        float *const in[2] = {from.I0, from.I1};
        float *out[2] = {};
        for (int k = 0; k < images; k++) out[k] = R.planes(to.nr, to.nc, C);
        for (int k = 0; k < images; k++) DO(R, pdeip_pyr_resize_dev(R.s, in[k], from.nr, from.nc, C, to.nr, to.nc, 0, out[k]));
        to.I0 = out[0];
        to.I1 = out[1];
    };
    auto smooth = [&](Level &lv) { // the scale's images replaced by their smoothed copies
        float *const in[2] = {lv.I0, lv.I1};
        float *out[2] = {};
        for (int k = 0; k < images; k++) out[k] = R.planes(lv.nr, lv.nc, C);
        for (int k = 0; k < images; k++) DO(R, pdeip_pyr_smooth_dev(R.s, in[k], lv.nr, lv.nc, C, G.data(), q.gsize, out[k]));
        lv.I0 = out[0];
        lv.I1 = out[1];
    };
    std::vector<Level> L(1);
    L[0].nr = nrows;
    L[0].nc = ncols;
    L[0].I0 = f0;
    L[0].I1 = f1;
    while ((int)L.size() < q.max_scales) {
        const Level cur = L.back();
        Level nx;
        nx.nr = (int)std::ceil(cur.nr * q.scl_factor);
        nx.nc = (int)std::ceil(cur.nc * q.scl_factor);
        resized(cur, nx);
        smooth(L.back());
        L.push_back(nx);
        if (nx.nr <= q.stop_rows || nx.nc <= q.stop_cols || (q.stop_when_stuck && nx.nr == cur.nr && nx.nc == cur.nc)) {
            if (q.smooth_last) smooth(L.back());
            break;
        }
    }
    return L;
}

// param.Us / param.Vs down the pyramid (:162-184): NaN -> 0, USap{scl} = imresize(USap{scl-1} .* scl_factor, scl_factor), doubles;
// every scale's field goes to the device as a double plane.  The coarsest one also starts the flow (:178, :183) -- MATLAB
// keeps that double array through the first firstLoop of the coarsest scale (`u_double` below); here, as in drivers.py, `start`
// receives its float32 rounding.
void apriori_pyramid(Run &R, const double *Us_host, std::vector<Level> &L, double scl_factor, bool second, float *start)
{
    if (Us_host == nullptr) return;
    std::vector<double> cur;
    for (size_t s = 0; s < L.size(); s++) {
        double *d = R.dplane(L[s].nr, L[s].nc);
        (second ? L[s].Vs : L[s].Us) = d;
        if (R.dry || R.rc != PDEIP_OK) continue;
        if (s == 0) {
            cur.assign(Us_host, Us_host + L[0].n());
            for (double &v : cur)
                if (v != v) v = 0.0;
        } else {
            std::vector<double> scaled(cur.size());
            for (size_t i = 0; i < cur.size(); i++) scaled[i] = cur[i] * scl_factor;
            cur = resize_double(scaled, L[s - 1].nr, L[s - 1].nc, L[s].nr, L[s].nc);
        }
        // `cur` is rewritten for the next scale: the copy must have left it
        DOHIP(R, hipMemcpyAsync(d, cur.data(), cur.size() * sizeof(double), hipMemcpyHostToDevice, R.s));
        DOHIP(R, hipStreamSynchronize(R.s));
    }
    if (R.dry || R.rc != PDEIP_OK) return;
    std::vector<float> f(cur.size());
    for (size_t i = 0; i < cur.size(); i++) f[i] = (float)cur[i];
    DOHIP(R, hipMemcpyAsync(start, f.data(), f.size() * sizeof(float), hipMemcpyHostToDevice, R.s));
    DOHIP(R, hipStreamSynchronize(R.s));
}

// First / second constancy images of a scale (:133-170): frame 0 and frame 1 of each term, [C1] and [C2] planes (C2 = 0: no second term)
struct Terms {
    const float *a0, *a1, *b0, *b1;
    int C1, C2;
    bool gradmag; // the second term takes second derivatives
};
Terms terms(Run &R, const Level &lv, int C, int fst, int snd)
{
    Terms t{lv.I0, lv.I1, nullptr, nullptr, C, 0, snd == PDEIP_TERM_GRADMAG};
    if (fst == PDEIP_TERM_GRAD) {
        float *g0 = R.planes(lv.nr, lv.nc, 2 * C), *g1 = R.planes(lv.nr, lv.nc, 2 * C);
        DO(R, pdeip_rgb2grad_dev(R.s, lv.I0, lv.nr, lv.nc, C, g0));
        DO(R, pdeip_rgb2grad_dev(R.s, lv.I1, lv.nr, lv.nc, C, g1));
        t.a0 = g0;
        t.a1 = g1;
        t.C1 = 2 * C;
    }
    if (snd != PDEIP_TERM_NONE) {
        t.b0 = lv.I0;
        t.b1 = lv.I1;
        t.C2 = C;
    }
    return t;
}

// The front half of a late-linearisation level: frame 1 of each term warped by the current field (w1, w2: written by the level's own
// warp, fused in the ND levels, coordinates + two bilinear warps in the AD level) and the derivatives against frame 0 --
// (Ix, Iy, It) of the first term, the same or (Ixt, Iyt, Ixx, Iyy, Ixy) of the second.
struct DataTerms {
    const Terms &t;
    int nr, nc;
    float *w1, *d1[3], *w2 = nullptr, *d2[5] = {};
    DataTerms(Run &R, const Level &lv, const Terms &terms) : t(terms), nr(lv.nr), nc(lv.nc)
    {
        w1 = R.planes(nr, nc, t.C1);
        for (auto &q : d1) q = R.planes(nr, nc, t.C1);
        if (t.C2 == 0) return;
        w2 = R.planes(nr, nc, t.C2);
        for (int k = 0; k < (t.gradmag ? 5 : 3); k++) d2[k] = R.planes(nr, nc, t.C2);
    }
    void first(Run &R) const { DO(R, pdeip_fst_derivatives5_dev(R.s, t.a0, w1, nr, nc, t.C1, d1[0], d1[1], d1[2])); }
    void second(Run &R) const
    {
        if (t.C2 == 0) return;
        if (t.gradmag) DO(R, pdeip_snd_derivatives5_dev(R.s, t.b0, w2, nr, nc, t.C2, d2[0], d2[1], d2[2], d2[3], d2[4]));
        else DO(R, pdeip_fst_derivatives5_dev(R.s, t.b0, w2, nr, nc, t.C2, d2[0], d2[1], d2[2]));
    }
    void derivatives(Run &R) const
    {
        first(R);
        second(R);
    }
};

// The unknowns of a late-linearisation run -- (U, V) or U alone -- and the other plane of each one's ping-pong.  A level takes the
// field in f and leaves it in f: whatever it swapped, alt is the plane that is free.
struct Fields {
    int nf = 0;
    float *f[2] = {}, *alt[2] = {};
};

// One scale of the flow driver: firstLoop x [warp, derivatives, secondLoop x (robust assembly + OPdiffWeights, a-priori terms,
// Oflow_sor_llin4_2d), median] -- FlowEminND_llin_2D_v10.m:208-356, flow_level.py FlowLlinLevel.run.
void flow_level(Run &R, const Params &p, const Level &lv, const Terms &t, Fields &F, double as_diff, bool u_double)
{
    const int nr = lv.nr, nc = lv.nc;
    const Solver solver{p.solver, p.iter, (float)p.omega};
    float *&U = F.f[0], *&V = F.f[1];
    const size_t m = R.mark();
    const DataTerms T(R, lv, t);
    float *coef[9]; // MGd, CuGd, CvGd, DuGd, DvGd, wW, wN, wE, wS
    for (auto &q : coef) q = R.planes(nr, nc);
    float *dUV = R.planes(nr, nc, 2), *dU = dUV, *dV = dUV + lv.n();
    for (int first = 0; first < p.firstLoop; first++) {
        DO(R, pdeip_flow_warp_dev(R.s, U, V, t.a1, t.C1, t.b1, t.C2, nr, nc, T.w1, T.w2));
        T.derivatives(R);
        DOHIP(R, hipMemsetAsync(dUV, 0, 2 * lv.n() * sizeof(float), R.s));
        for (int k = 0; k < p.secondLoop; k++) {
            // weights come back in wW wN wS wE order (OPdiffWeights, :389-433)
            DO(R, pdeip_flow_assemble_weights_dev(R.s, T.d1[0], T.d1[1], T.d1[2], t.C1, (float)p.b1, T.d2[0], T.d2[1], T.d2[2], T.d2[3], T.d2[4], t.C2, (float)p.b2, U, V, dU,
                                                  dV, (float)p.alpha, nr, nc, coef[0], coef[1], coef[2], coef[3], coef[4], coef[5], coef[6], coef[8], coef[7]));
            if (lv.Us) DO(R, pdeip_flow_apriori_dev(R.s, lv.Us, U, dU, p.gammaS, p.alpha, as_diff, u_double && first == 0, k == 0, nr, nc, coef[1], coef[3]));
            if (lv.Vs) DO(R, pdeip_flow_apriori_dev(R.s, lv.Vs, V, dV, p.gammaS, p.alpha, as_diff, u_double && first == 0, k == 0, nr, nc, coef[2], coef[4]));
            solve_flow_llin4(R, solver, U, V, dU, dV, coef, nr, nc);
        }
        DO(R, pdeip_median3_pair_dev(R.s, U, dU, V, dV, nr, nc, F.alt[0], F.alt[1]));
        std::swap(F.f[0], F.alt[0]);
        std::swap(F.f[1], F.alt[1]);
    }
    R.release(m);
}

// The anisotropic-diffusion twin: FlowEminAD_llin_2D_v10.m:198-366, flow_level.py FlowAdLevel.run -- eight ADdiffWeights from the
// image (`flow_diffusion` false: once per level, from frame 0 of the scale) or from U+dU+V+dV (true: every inner iteration), and
// Oflow_sor_llin8_2d.
void flow_ad_level(Run &R, const Params &p, const Level &lv, int C, const Terms &t, double quantile, bool flow_diffusion, Fields &F, double as_diff, bool u_double)
{
    const int nr = lv.nr, nc = lv.nc;
    const Solver solver{p.solver, p.iter, (float)p.omega};
    float *&U = F.f[0], *&V = F.f[1];
    const size_t m = R.mark();
    float *X = R.planes(nr, nc), *Y = R.planes(nr, nc), *S = R.planes(nr, nc);
    const DataTerms T(R, lv, t);
    float *coef[5], *w8[8], *dU = R.planes(nr, nc), *dV = R.planes(nr, nc); // MGd, CuGd, CvGd, DuGd, DvGd | wW, wNW, wN, wNE, wE, wSE, wS, wSW
    for (auto &q : coef) q = R.planes(nr, nc);
    for (auto &q : w8) q = R.planes(nr, nc);
    if (!flow_diffusion) DO(R, pdeip_ad_weights_dev(R.s, lv.I0, nr, nc, C, quantile, w8[0], w8[1], w8[2], w8[3], w8[4], w8[5], w8[6], w8[7]));
    for (int first = 0; first < p.firstLoop; first++) {
        DO(R, pdeip_flow_coords_dev(R.s, U, V, nr, nc, X, Y));
        DO(R, pdeip_warp_bilinear_dev(R.s, t.a1, X, Y, nr, nc, t.C1, T.w1));
        T.first(R); // between the two warps, as FlowAdLevel.run has it
        if (t.C2 > 0) DO(R, pdeip_warp_bilinear_dev(R.s, t.b1, X, Y, nr, nc, t.C2, T.w2));
        T.second(R);
        DOHIP(R, hipMemsetAsync(dU, 0, lv.n() * sizeof(float), R.s));
        DOHIP(R, hipMemsetAsync(dV, 0, lv.n() * sizeof(float), R.s));
        for (int k = 0; k < p.secondLoop; k++) {
            if (t.C2 > 0 && t.gradmag)
                DO(R, pdeip_flow_assemble_gradmag_dev(R.s, T.d1[0], T.d1[1], T.d1[2], t.C1, (float)p.b1, T.d2[0], T.d2[1], T.d2[2], T.d2[3], T.d2[4], t.C2, (float)p.b2, dU, dV,
                                                      (float)p.alpha, nr, nc, coef[0], coef[1], coef[2], coef[3], coef[4]));
            else // without a second term T.d2 is null
                DO(R, pdeip_flow_assemble_dev(R.s, T.d1[0], T.d1[1], T.d1[2], t.C1, (float)p.b1, T.d2[0], T.d2[1], T.d2[2], t.C2, t.C2 > 0 ? (float)p.b2 : 0.0f, dU, dV,
                                              (float)p.alpha, nr, nc, coef[0], coef[1], coef[2], coef[3], coef[4]));
            if (lv.Us) DO(R, pdeip_flow_apriori_dev(R.s, lv.Us, U, dU, p.gammaS, p.alpha, as_diff, u_double && first == 0, k == 0, nr, nc, coef[1], coef[3]));
            if (lv.Vs) DO(R, pdeip_flow_apriori_dev(R.s, lv.Vs, V, dV, p.gammaS, p.alpha, as_diff, u_double && first == 0, k == 0, nr, nc, coef[2], coef[4]));
            if (flow_diffusion) { // U+dU+V+dV, left to right
                DO(R, pdeip_add_dev(R.s, U, dU, nr, nc, S));
                DO(R, pdeip_add_dev(R.s, S, V, nr, nc, S));
                DO(R, pdeip_add_dev(R.s, S, dV, nr, nc, S));
                DO(R, pdeip_ad_weights_dev(R.s, S, nr, nc, 1, quantile, w8[0], w8[1], w8[2], w8[3], w8[4], w8[5], w8[6], w8[7]));
            }
            solve_flow_llin8_or_4(R, solver, U, V, dU, dV, coef, w8, nr, nc);
        }
        DO(R, pdeip_median3_dev(R.s, U, dU, nr, nc, F.alt[0]));
        DO(R, pdeip_median3_dev(R.s, V, dV, nr, nc, F.alt[1]));
        std::swap(F.f[0], F.alt[0]);
        std::swap(F.f[1], F.alt[1]);
    }
    R.release(m);
}

// The stereo twin: DispEminND_llin_2D.m:202-316, flow_level.py DispLlinLevel.run
void disp_level(Run &R, const Params &p, const Level &lv, const Terms &t, Fields &F, double as_diff, bool u_double)
{
    const int nr = lv.nr, nc = lv.nc;
    const Solver solver{p.solver, p.iter, (float)p.omega};
    float *&U = F.f[0];
    const size_t m = R.mark();
    const DataTerms T(R, lv, t);
    float *CuGd = R.planes(nr, nc), *DuGd = R.planes(nr, nc), *S = R.planes(nr, nc), *w[4], *dU = R.planes(nr, nc);
    for (auto &q : w) q = R.planes(nr, nc); // wW, wN, wE, wS
    for (int first = 0; first < p.firstLoop; first++) {
        DO(R, pdeip_flow_warp_dev(R.s, U, nullptr, t.a1, t.C1, t.b1, t.C2, nr, nc, T.w1, T.w2)); // along x only
        T.derivatives(R);
        DOHIP(R, hipMemsetAsync(dU, 0, lv.n() * sizeof(float), R.s));
        for (int k = 0; k < p.secondLoop; k++) {
            if (t.C2 > 0 && t.gradmag) // (Ixt, Iyt, Ixx, Ixy)
                DO(R, pdeip_disp_assemble_gradmag_dev(R.s, T.d1[0], T.d1[1], t.C1, (float)p.b1, T.d2[0], T.d2[1], T.d2[2], T.d2[4], t.C2, (float)p.b2, dU, (float)p.alpha, nr, nc, CuGd, DuGd));
            else
                DO(R, pdeip_disp_assemble_dev(R.s, T.d1[0], T.d1[1], t.C1, (float)p.b1, T.d2[0], T.d2[1], t.C2, t.C2 > 0 ? (float)p.b2 : 0.0f, dU, (float)p.alpha, nr, nc, CuGd, DuGd));
            if (lv.Us) DO(R, pdeip_disp_apriori_dev(R.s, lv.Us, U, dU, p.gammaS, p.alpha, as_diff, u_double && first == 0, k == 0, nr, nc, CuGd, DuGd));
            DO(R, pdeip_add_dev(R.s, U, dU, nr, nc, S));
            DO(R, pdeip_diffweights6_dev(R.s, S, nr, nc, 1, 0.00001f, w[0], w[1], w[2], w[3]));
            solve_disp_llin4(R, solver, U, dU, CuGd, DuGd, w, nr, nc);
        }
        DO(R, pdeip_median3_dev(R.s, U, dU, nr, nc, F.alt[0]));
        std::swap(F.f[0], F.alt[0]);
    }
    R.release(m);
}

// The scale loop of the late-linearisation drivers (FlowEminND_llin_2D_v10.m:100-369, FlowEminAD_llin_2D_v10.m, DispEminND_llin_2D.m:77-316;
// drivers.py _flow_llin_planes / DispEminND_llin_2D): frames up and ./255, the pyramid down to min_size, a zero start unless an a-priori
// field starts it, the a-priori pyramids; from the coarsest scale on [constancy images, the driver's level, field .* (1/scl_factor)
// resized to the finer scale]; results down.  What a driver brings of its own:
struct Llin {
    const float *Ia, *Ib;     // both frames in Ia (Ib null), or the left and the right image
    int nf;                   // fields: U, V of a flow, U of a disparity
    const double *apriori[2]; // param.Us, param.Vs (or null)
    int min_size;             // the pyramid's last scale
    double as_diff0;          // asDiff = as_diff0 * scl_factor^k at scale k (0: the finest) of the a-priori term
    float *out[2];
};
// level(lv, t, F, as_diff, u_double): the driver's level on F
template <class LevelBody> void llin_driver(Run &R, const Llin &d, int nrows, int ncols, int C, int fst, int snd, const Params &p, LevelBody level)
{
    float *fr = upload_frames(R, d.Ia, d.Ib, nrows, ncols, C, true);
    std::vector<Level> L = build_pyramid(R, 2, fr, fr + (size_t)C * nrows * ncols, nrows, ncols, C, {p.scl_factor, p.scales, d.min_size, d.min_size, true, 5, 1.25, false});
    const int last = (int)L.size() - 1;
    Fields F;
    F.nf = d.nf;
    for (int k = 0; k < F.nf; k++) F.f[k] = zero_plane(R, L[last].nr, L[last].nc);
    for (int k = 0; k < F.nf; k++) F.alt[k] = R.planes(L[last].nr, L[last].nc);
    for (int k = 0; k < F.nf; k++) apriori_pyramid(R, d.apriori[k], L, p.scl_factor, k == 1, F.f[k]);
    const bool apriori = d.apriori[0] != nullptr || d.apriori[1] != nullptr;
    const float inv = (float)(1.0 / p.scl_factor);
    for (int s = last; s >= 0; s--) {
        const size_t m = R.mark();
        const Terms t = terms(R, L[s], C, fst, snd);
        level(L[s], t, F, d.as_diff0 * std::pow(p.scl_factor, (double)s), s == last && apriori);
        if (s > 0) { // U = imresize(U .* (1/scl_factor), size of the finer scale, 'triangle')
            const Level &f = L[s - 1];
            for (int k = 0; k < F.nf; k++) scale(R, F.alt[k], F.f[k], L[s].n(), inv, false);
            R.release(m); // the finer planes may reuse what this scale's terms held; the fields lie below the mark
            const Fields coarse = F;
            for (int k = 0; k < F.nf; k++) F.f[k] = R.planes(f.nr, f.nc);
            for (int k = 0; k < F.nf; k++) F.alt[k] = R.planes(f.nr, f.nc);
            for (int k = 0; k < F.nf; k++) DO(R, pdeip_pyr_resize_dev(R.s, coarse.alt[k], L[s].nr, L[s].nc, 1, f.nr, f.nc, 0, F.f[k]));
        }
    }
    download(R, {{d.out[0], F.f[0]}, {d.out[1], F.f[1]}}, L[0].n());
}

// DispEminND_llin_sym_2D.m:51-275 (runme.m:28): symmetric stereo -- both views' disparities at once, each warped into the other for
// the symmetry term.  flow_level.py DispSymLevel.run / drivers.py DispEminND_llin_sym_2D are the statement the tests compare with
// (same `_dev` stages, same order).  No division by 255 in this driver (:81-82), a 3 x 3 Gaussian, coarsest scale unsmoothed.
void sym_level(Run &R, const SymParams &p, const Level &lv, int C, float *(&U)[2], double sr_diff)
{
    const int nr = lv.nr, nc = lv.nc;
    const size_t n = lv.n();
    const double kS = C * p.beta / p.alpha, sr2 = std::pow(sr_diff, 2.0);
    const float *I[2] = {lv.I0, lv.I1};
    float *zero = R.planes(nr, nc), *X = R.planes(nr, nc), *Y = R.planes(nr, nc), *S = R.planes(nr, nc);
    float *warped[2], *der[2][8], *CuG[2], *DuG[2], *w[2][4], *Un[2], *dU[2];
    double *Uw[2], *sym[2][4];
    for (int v = 0; v < 2; v++) {
        warped[v] = R.planes(nr, nc, C);
        for (auto &q : der[v]) q = R.planes(nr, nc, C);
        CuG[v] = R.planes(nr, nc);
        DuG[v] = R.planes(nr, nc);
        for (auto &q : w[v]) q = R.planes(nr, nc);
        Un[v] = R.planes(nr, nc);
        dU[v] = R.planes(nr, nc);
        Uw[v] = R.dplane(nr, nc);
        for (auto &q : sym[v]) q = R.dplane(nr, nc);
    }
    DOHIP(R, hipMemsetAsync(zero, 0, n * sizeof(float), R.s));
    for (int fl = 0; fl < p.firstLoop; fl++) {
        for (int v = 0; v < 2; v++) { // view v: own image, the other view warped by U{v}
            DO(R, pdeip_flow_coords_dev(R.s, U[v], zero, nr, nc, X, Y));
            DO(R, pdeip_warp_bilinear_dev(R.s, I[1 - v], X, Y, nr, nc, C, warped[v]));
        }
        DO(R, pdeip_sym_warp_flow_dev(R.s, U[0], U[1], nr, nc, Uw[0]));
        DO(R, pdeip_sym_warp_flow_dev(R.s, U[1], U[0], nr, nc, Uw[1]));
        for (int v = 0; v < 2; v++) {
            DO(R, pdeip_fst_derivatives5_dev(R.s, I[v], warped[v], nr, nc, C, der[v][0], der[v][1], der[v][2]));
            DO(R, pdeip_snd_derivatives5_dev(R.s, I[v], warped[v], nr, nc, C, der[v][3], der[v][4], der[v][5], der[v][6], der[v][7]));
            DO(R, pdeip_sym_flow_terms_dev(R.s, U[v], Uw[1 - v], nr, nc, sym[v][0], sym[v][1], sym[v][2], sym[v][3]));
            DOHIP(R, hipMemsetAsync(dU[v], 0, n * sizeof(float), R.s));
        }
        for (int k = 0; k < p.secondLoop; k++) {
            for (int v = 0; v < 2; v++) {
                DO(R, pdeip_sym_assemble_dev(R.s, der[v][0], der[v][1], der[v][3], der[v][4], der[v][5], der[v][7], C, sym[v][0], sym[v][1], sym[v][2], sym[v][3], dU[v],
                                             (float)p.b1, (float)p.b2, (float)p.alpha, kS, sr2, k == 0 ? 1 : 0, nr, nc, CuG[v], DuG[v]));
                DO(R, pdeip_add_dev(R.s, U[v], dU[v], nr, nc, S));
                DO(R, pdeip_diffweights6_dev(R.s, S, nr, nc, 1, (float)0.00001, w[v][0], w[v][1], w[v][2], w[v][3]));
            }
            // both views in one call, which takes param.solver itself
            DO(R, pdeip_disp_sor_llin_sym4_dev(R.s, U[0], dU[0], CuG[0], DuG[0], w[0][0], w[0][1], w[0][2], w[0][3], U[1], dU[1], CuG[1], DuG[1], w[1][0], w[1][1],
                                               w[1][2], w[1][3], nr, nc, p.iter, (float)p.omega, p.solver, R.mode, 0));
        }
        for (int v = 0; v < 2; v++) {
            DO(R, pdeip_median3_dev(R.s, U[v], dU[v], nr, nc, Un[v]));
            std::swap(U[v], Un[v]);
        }
    }
}
void disp_sym(Run &R, const float *Il, const float *Ir, int nrows, int ncols, int C, const SymParams &p, float *U_out)
{
    const size_t n = (size_t)nrows * ncols;
    float *fr = upload_frames(R, Il, Ir, nrows, ncols, C, false);
    const std::vector<Level> L = build_pyramid(R, 2, fr, fr + C * n, nrows, ncols, C, {p.scl_factor, ALL_SCALES, 10, 10, false, 3, 1.0, false});
    const Level top = L.back();
    float *U[2] = {zero_plane(R, top.nr, top.nc), zero_plane(R, top.nr, top.nc)};
    const float inv = (float)(1.0 / p.scl_factor);
    for (int s = (int)L.size() - 1; s >= 0; s--) {
        // the level gets its own copies of the two fields (the Python level clones them): its ping-pong may end in either plane set
        float *W[2] = {R.planes(L[s].nr, L[s].nc), R.planes(L[s].nr, L[s].nc)};
        for (int v = 0; v < 2; v++) DO(R, copy_d2d(R.s, W[v], U[v], L[s].n()));
        sym_level(R, p, L[s], C, W, 2.0 * std::pow(1.0 / p.scl_factor, (double)(-s))); // srDiff = 2*(1/scl_factor)^-(scl-1), scl 1-based there
        U[0] = W[0];
        U[1] = W[1];
        if (s > 0) {
            const Level &f = L[s - 1];
            for (int v = 0; v < 2; v++) {
                float *sc = R.planes(L[s].nr, L[s].nc), *up = R.planes(f.nr, f.nc);
                scale(R, sc, U[v], L[s].n(), inv, false);
                DO(R, pdeip_pyr_resize_dev(R.s, sc, L[s].nr, L[s].nc, 1, f.nr, f.nc, 0, up));
                U[v] = up;
            }
        }
    }
    download(R, {{U_out, U[0]}, {U_out + n, U[1]}}, n);
}

// FlowEminHS_elin_2D_v10.m:52-200 (runme.m:74): Horn-Schunck with early linearisation.  Per scale the data terms from the unwarped
// frames (k_hs_assemble), a constant diffusion weight alpha * channels and ONE Oflow_sor_elin4_2d call; between scales
// imresize(medfilt2(U .* (1/scl_factor)), 'OutputSize', ...) with imresize's default, bicubic, kernel (:189-190).  drivers.py
// FlowEminHS_elin_2D_v10 / flow_level.py FlowHsLevel are the statement the tests compare with.
void flow_hs(Run &R, const float *Iin, int nrows, int ncols, int C, const Params &p, float *U_out, float *V_out)
{
    const size_t n = (size_t)nrows * ncols;
    float *fr = upload_frames(R, Iin, nullptr, nrows, ncols, C, true);
    const std::vector<Level> L = build_pyramid(R, 2, fr, fr + C * n, nrows, ncols, C, {p.scl_factor, p.scales, 20, 20, true, 5, 1.25, false});
    const Level top = L.back();
    float *U = zero_plane(R, top.nr, top.nc), *V = zero_plane(R, top.nr, top.nc);
    const float inv = (float)(1.0 / p.scl_factor);
    for (int s = (int)L.size() - 1; s >= 0; s--) {
        const int nr = L[s].nr, nc = L[s].nc;
        float *W = R.planes(nr, nc), *coef[9]; // MGd, CuGd, CvGd, DuGd, DvGd and four times W
        for (int k = 0; k < 9; k++) coef[k] = k < 5 ? R.planes(nr, nc) : W;
        DO(R, pdeip_hs_assemble_dev(R.s, L[s].I0, L[s].I1, C, (float)p.b1, (float)p.b2, nr, nc, coef[0], coef[1], coef[2], coef[3], coef[4]));
        fill(R, W, L[s].n(), (float)(p.alpha * C)); // W = alpha*channels*ones (:121)
        if (p.iter > 0) solve_elin4(R, {p.solver, p.iter, (float)p.omega}, U, V, coef, nr, nc);
        if (s > 0) {
            const Level &f = L[s - 1];
            float *sU = R.planes(nr, nc), *sV = R.planes(nr, nc), *mU = R.planes(nr, nc), *mV = R.planes(nr, nc);
            scale(R, sU, U, L[s].n(), inv, false);
            scale(R, sV, V, L[s].n(), inv, false);
            DO(R, pdeip_median3_dev(R.s, sU, nullptr, nr, nc, mU));
            DO(R, pdeip_median3_dev(R.s, sV, nullptr, nr, nc, mV));
            U = R.planes(f.nr, f.nc);
            V = R.planes(f.nr, f.nc);
            DO(R, pdeip_pyr_resize_dev(R.s, mU, nr, nc, 1, f.nr, f.nc, 1, U));
            DO(R, pdeip_pyr_resize_dev(R.s, mV, nr, nc, 1, f.nr, f.nc, 1, V));
        }
    }
    download(R, {{U_out, U}, {V_out, V}}, n);
}

// TV-L1 flow (this library's own driver; include/pdeip.h has the contract, drivers.py FlowTVL1 / flow_level.py FlowTvl1Level are the
// statement the tests compare with): the late-linearisation drivers' pyramid and scale loop around a level of `warps` x [warp,
// derivatives, rc, `iter` primal-dual iterations, median].  The duals start a scale at zero and persist from warp to warp within it.
struct Tvl1Params {
    double lambda, huber, tau, sigma, scl_factor;
    int warps, iter, scales;
};
void tvl1_level(Run &R, const Tvl1Params &p, const Level &lv, Fields &F)
{
    const int nr = lv.nr, nc = lv.nc;
    const size_t m = R.mark();
    float *W = R.planes(nr, nc), *gt = R.planes(nr, nc), *gx = R.planes(nr, nc), *gy = R.planes(nr, nc), *rc = R.planes(nr, nc);
    float *P = R.planes(nr, nc, 4), *iu = R.planes(nr, nc), *iv = R.planes(nr, nc);
    const pdeip_tvl1_params prm{p.lambda, p.huber, p.iter, p.tau, p.sigma};
    DOHIP(R, hipMemsetAsync(P, 0, 4 * lv.n() * sizeof(float), R.s));
    for (int w = 0; w < p.warps; w++) {
        DO(R, pdeip_flow_warp_dev(R.s, F.f[0], F.f[1], lv.I1, 1, nullptr, 0, nr, nc, W, nullptr));
        DO(R, pdeip_fst_derivatives5_dev(R.s, lv.I0, W, nr, nc, 1, gt, gx, gy)); // Idt has the reference's sign and scale: not used
        DO(R, pdeip_tvl1_rc_dev(R.s, lv.I0, W, gx, gy, F.f[0], F.f[1], nr, nc, rc));
        DO(R, pdeip_tvl1_iterate_dev(R.s, rc, gx, gy, F.f[0], F.f[1], P, nr, nc, &prm, iu, iv));
        DO(R, pdeip_median3_pair_dev(R.s, iu, nullptr, iv, nullptr, nr, nc, F.alt[0], F.alt[1]));
        std::swap(F.f[0], F.alt[0]);
        std::swap(F.f[1], F.alt[1]);
    }
    R.release(m);
}
void flow_tvl1(Run &R, const float *Iin, int nrows, int ncols, const Tvl1Params &p, float *U_out, float *V_out)
{
    float *fr = upload_frames(R, Iin, nullptr, nrows, ncols, 1, true);
    const std::vector<Level> L = build_pyramid(R, 2, fr, fr + (size_t)nrows * ncols, nrows, ncols, 1, {p.scl_factor, p.scales, 20, 20, true, 5, 1.25, false});
    const int last = (int)L.size() - 1;
    Fields F;
    F.nf = 2;
    for (int k = 0; k < 2; k++) F.f[k] = zero_plane(R, L[last].nr, L[last].nc);
    for (int k = 0; k < 2; k++) F.alt[k] = R.planes(L[last].nr, L[last].nc);
    DO(R, tvl1_reserve(nrows, ncols)); // the iteration's workspace grows once, before the first launch that uses it
    const float inv = (float)(1.0 / p.scl_factor);
    for (int s = last; s >= 0; s--) {
        const size_t m = R.mark();
        tvl1_level(R, p, L[s], F);
        if (s > 0) { // U = imresize(U .* (1/scl_factor), size of the finer scale, 'triangle'), as llin_driver has it
            const Level &f = L[s - 1];
            for (int k = 0; k < 2; k++) scale(R, F.alt[k], F.f[k], L[s].n(), inv, false);
            R.release(m);
            const Fields coarse = F;
            for (int k = 0; k < 2; k++) F.f[k] = R.planes(f.nr, f.nc);
            for (int k = 0; k < 2; k++) F.alt[k] = R.planes(f.nr, f.nc);
            for (int k = 0; k < 2; k++) DO(R, pdeip_pyr_resize_dev(R.s, coarse.alt[k], L[s].nr, L[s].nc, 1, f.nr, f.nc, 0, F.f[k]));
        }
    }
    download(R, {{U_out, F.f[0]}, {V_out, F.f[1]}}, L[0].n());
}

// FlowEminNDFASFMG_elin_2D_v10.m (runme.m:90): FAS full-multigrid flow with early linearisation.  Image pyramid by halving
// (:104-120), per-scale derivative planes and constants (:125-153), per scale, coarse to fine (:161-183), one FAS V- or W-cycle
// (FAS_CYCLE, :193-273) whose smoother (:367-464) is firstLoop x [robust data weights + OPdiffWeights, Oflow_sor_elin4_2d];
// residuals through the solver's residual operator, the coarse right-hand side through Oflow_lhs_elin4_2d, full-weighting
// restriction, bilinear prolongation of the correction, bicubic up-scaling of the flow between scales.  fas.py FasFmgFlow is the
// statement the tests compare with: the same `_dev` stages in the same order.
struct FasScale {
    int nr, nc;
    float *pl; // [13][C][nc][nr]: Idt, Idx, Idy, Idxx, Idyy, Idxy, Idxt, Idyt, M, Cu, Cv, Du, Dv
};
struct Fas {
    Run &R;
    const FasParams &p;
    int C;
    std::vector<FasScale> S;
    float *plane(int s, int k) const { return S[s].pl + (size_t)k * C * S[s].nr * S[s].nc; }
    // in place on U, V; RU, RV ([C] planes) receive the residuals when given
    void smooth(int s, float *U, float *V, const float *Cu, const float *Cv, float *RU, float *RV)
    {
        const int nr = S[s].nr, nc = S[s].nc;
        const size_t m = R.mark();
        float *coef[9]; // MGd CuGd CvGd DuGd DvGd wW wN wE wS
        for (auto &q : coef) q = R.planes(nr, nc);
        for (int it = 0; it < p.firstLoop; it++) { // robust data weights (:377-397) and OPdiffWeights(U, V) (:392): wW wN wS wE order
            DO(R, pdeip_fas_assemble_weights_dev(R.s, S[s].pl, Cu, Cv, U, V, nr, nc, C, (float)p.b1, (float)p.b2, (float)(C * p.alpha), coef[0], coef[1], coef[2], coef[3], coef[4],
                                                 coef[5], coef[6], coef[8], coef[7]));
            solve_elin4(R, {p.solver, p.iter, (float)p.omega}, U, V, coef, nr, nc);
        }
        if (RU != nullptr) {
            float *f[5];
            for (auto &q : f) q = R.planes(nr, nc, C);
            DO(R, pdeip_fas_assemble_dev(R.s, S[s].pl, Cu, Cv, U, V, nr, nc, C, (float)p.b1, (float)p.b2, (float)p.alpha, 1, f[0], f[1], f[2], f[3], f[4], nullptr));
            DO(R, pdeip_flow_opdiffweights_dev(R.s, U, V, nullptr, nullptr, nr, nc, coef[5], coef[6], coef[8], coef[7]));
            DO(R, pdeip_oflow_res_elin4_dev(R.s, RU, RV, U, V, f[0], f[1], f[2], f[3], f[4], coef[5], coef[6], coef[7], coef[8], nr, nc, C));
        }
        R.release(m);
    }
    // one V (cycle_index 1) or W (2) cycle at scale s on U, V (in place); Cu / Cv: the scale's own or the cycle's right-hand side
    void cycle(int s, float *U, float *V, const float *Cu, const float *Cv)
    {
        if (s == (int)S.size() - 1) {
            smooth(s, U, V, Cu, Cv, nullptr, nullptr);
            return;
        }
        const int nr = S[s].nr, nc = S[s].nc, cr = S[s + 1].nr, cc = S[s + 1].nc;
        const float sf = (float)p.scl_factor;
        for (int ci = 0; ci < p.cycle_index; ci++) {
            const size_t m = R.mark();
            float *RU = R.planes(nr, nc, C), *RV = R.planes(nr, nc, C);
            smooth(s, U, V, Cu, Cv, RU, RV);
            float *RUres = R.planes(cr, cc, C), *RVres = R.planes(cr, cc, C), *Ures = R.planes(cr, cc), *Vres = R.planes(cr, cc);
            DO(R, pdeip_fas_restrict_dev(R.s, RU, nr, nc, C, sf, RUres));
            DO(R, pdeip_fas_restrict_dev(R.s, RV, nr, nc, C, sf, RVres));
            DO(R, pdeip_fas_restrict_dev(R.s, U, nr, nc, 1, sf, Ures));
            DO(R, pdeip_fas_restrict_dev(R.s, V, nr, nc, 1, sf, Vres));
            float *MGd = R.planes(cr, cc, C), *DuGd = R.planes(cr, cc, C), *DvGd = R.planes(cr, cc, C), *gd = R.planes(cr, cc, C), *w[4];
            for (auto &q : w) q = R.planes(cr, cc); // wW wN wE wS
            DO(R, pdeip_fas_assemble_dev(R.s, S[s + 1].pl, nullptr, nullptr, Ures, Vres, cr, cc, C, (float)p.b1, (float)p.b2, (float)p.alpha, 1, MGd, nullptr, nullptr, DuGd, DvGd, gd));
            DO(R, pdeip_flow_opdiffweights_dev(R.s, Ures, Vres, nullptr, nullptr, cr, cc, w[0], w[1], w[3], w[2]));
            float *Au = R.planes(cr, cc, C), *Av = R.planes(cr, cc, C), *fu = R.planes(cr, cc, C), *fv = R.planes(cr, cc, C);
            DO(R, pdeip_oflow_lhs_elin4_dev(R.s, Au, Av, Ures, Vres, MGd, DuGd, DvGd, w[0], w[1], w[2], w[3], cr, cc, C));
            DO(R, pdeip_fas_rhs_dev(R.s, RUres, Au, gd, cr, cc, C, fu));
            DO(R, pdeip_fas_rhs_dev(R.s, RVres, Av, gd, cr, cc, C, fv));
            float *Uc = R.planes(cr, cc), *Vc = R.planes(cr, cc);
            DO(R, copy_d2d(R.s, Uc, Ures, (size_t)cr * cc));
            DO(R, copy_d2d(R.s, Vc, Vres, (size_t)cr * cc));
            cycle(s + 1, Uc, Vc, fu, fv);
            DO(R, pdeip_fas_prolong_add_dev(R.s, U, nr, nc, Uc, Ures, cr, cc, (float)(1.0 / p.scl_factor)));
            DO(R, pdeip_fas_prolong_add_dev(R.s, V, nr, nc, Vc, Vres, cr, cc, (float)(1.0 / p.scl_factor)));
            R.release(m);
        }
        smooth(s, U, V, Cu, Cv, nullptr, nullptr);
    }
};
void fas_fmg(Run &R, const float *Iin, int nrows, int ncols, int C, const FasParams &p, float *U_out, float *V_out)
{
    const size_t n = (size_t)nrows * ncols;
    float *up = upload_frames(R, Iin, nullptr, nrows, ncols, C, false); // 0..255: this driver does not rescale
    // fspecial('gaussian', [5 5], 1) in single.  fas.py also zeroes what lies below eps * max before it divides by the sum, as fspecial
    // does: at 5 x 5 and sigma 1 the smallest value is exp(-4), so this is the pyramid's mask.
    constexpr int GSIZE = 5; // what pdeip_fas_gauss5_dev takes
    constexpr double SIGMA = 1.0;
    // the corner is exp(-r^2 / sigma^2) of the centre, r = GSIZE / 2, and eps is exp(-36.04): beyond that the zeroing would have to be stated here
    static_assert((GSIZE / 2) * (GSIZE / 2) / (SIGMA * SIGMA) < 36.0, "fas.py zeroes mask values below eps * max; gaussian_mask does not");
    const std::vector<double> g = gaussian_mask(GSIZE, SIGMA);
    float G[GSIZE * GSIZE];
    for (int i = 0; i < GSIZE * GSIZE; i++) G[i] = (float)g[i];
    struct Img {
        int nr, nc;
        float *a, *b;
    };
    std::vector<Img> P(1);
    P[0] = {nrows, ncols, R.planes(nrows, ncols, C), R.planes(nrows, ncols, C)};
    DO(R, pdeip_fas_gauss5_dev(R.s, up, nrows, ncols, C, G, P[0].a));
    DO(R, pdeip_fas_gauss5_dev(R.s, up + C * n, nrows, ncols, C, G, P[0].b));
    while ((int)P.size() < p.scales) {
        const Img cur = P.back();
        Img nx{(cur.nr + 1) / 2, (cur.nc + 1) / 2, nullptr, nullptr};
        nx.a = R.planes(nx.nr, nx.nc, C);
        nx.b = R.planes(nx.nr, nx.nc, C);
        DO(R, pdeip_fas_down_dev(R.s, cur.a, cur.nr, cur.nc, C, nx.a));
        DO(R, pdeip_fas_down_dev(R.s, cur.b, cur.nr, cur.nc, C, nx.b));
        P.push_back(nx);
        if (nx.nr <= 10 || nx.nc <= 10) break;
    }
    Fas F{R, p, C, {}};
    for (const Img &im : P) {
        FasScale sc{im.nr, im.nc, R.planes(im.nr, im.nc, 13 * C)};
        DO(R, pdeip_fas_prepare_dev(R.s, im.a, im.b, im.nr, im.nc, C, (float)p.b1, (float)p.b2, sc.pl));
        F.S.push_back(sc);
    }
    const int last = (int)F.S.size() - 1;
    float *U = zero_plane(R, F.S[last].nr, F.S[last].nc), *V = zero_plane(R, F.S[last].nr, F.S[last].nc);
    for (int s = last; s >= 0; s--) {
        F.cycle(s, U, V, F.plane(s, 9), F.plane(s, 10)); // the scale's own Cu, Cv
        if (s > 0) {
            float *Un = R.planes(F.S[s - 1].nr, F.S[s - 1].nc), *Vn = R.planes(F.S[s - 1].nr, F.S[s - 1].nc);
            DO(R, pdeip_fas_upscale_dev(R.s, U, F.S[s].nr, F.S[s].nc, (float)(1.0 / p.scl_factor), F.S[s - 1].nr, F.S[s - 1].nc, Un));
            DO(R, pdeip_fas_upscale_dev(R.s, V, F.S[s].nr, F.S[s].nc, (float)(1.0 / p.scl_factor), F.S[s - 1].nr, F.S[s - 1].nc, Vn));
            U = Un;
            V = Vn;
        }
    }
    download(R, {{U_out, U}, {V_out, V}}, n);
}

// TVdenoise8.m:36-111 / TVdenoise4.m:37-114: a short pyramid (down to scl x the frame), per scale the lagged-diffusivity loop --
// outer_iter + 1 times [diffusion weights of the current estimate, PsiData / TRACE / B, PDEsolver8 | PDEsolver4] --, the
// estimate resized up to the next finer scale.  drivers.py `_tv` / flow_level.py TvLevel, Tv4Level are the statement the tests
// compare with.  TVdenoise8 leaves its coarsest scale unsmoothed.
void tv_run(Run &R, const float *Iin, int nrows, int ncols, int F, const TvParams &p, bool eight, float *Iout_host)
{
    const size_t n0 = (size_t)nrows * ncols * F;
    float *I = R.planes(nrows, ncols, F);
    DOHIP(R, hipMemcpyAsync(I, Iin, n0 * sizeof(float), hipMemcpyHostToDevice, R.s));
    const std::vector<Level> L = build_pyramid(R, 1, I, nullptr, nrows, ncols, F,
                                               {p.scl_factor, ALL_SCALES, (int)std::ceil(nrows * p.scl), (int)std::ceil(ncols * p.scl), !eight, eight ? 5 : 7, eight ? 1.25 : 2.0, true});
    const Solver solver{p.solver, p.inner_iter, (float)p.omega};
    const float *est = L.back().I0;
    for (int s = (int)L.size() - 1; s >= 0; s--) {
        const int nr = L[s].nr, nc = L[s].nc;
        float *X = R.planes(nr, nc, F), *TRACE = R.planes(nr, nc, F), *B = R.planes(nr, nc, F), *w[8] = {};
        for (int k = 0; k < (eight ? 8 : 4); k++) w[k] = R.planes(nr, nc, F);
        DO(R, copy_d2d(R.s, X, est, L[s].n() * F));
        for (int it = 0; it <= p.outer_iter; it++) { // for iter=0:param.outer_iter
            if (eight) {
                DO(R, pdeip_tv_assemble_dev(R.s, X, L[s].I0, nr, nc, F, (float)p.alpha, TRACE, B, w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]));
                solve_pde8(R, solver, X, TRACE, B, w, nr, nc, F);
            } else {
                DO(R, pdeip_tv4_assemble_dev(R.s, X, L[s].I0, nr, nc, F, (float)p.alpha, TRACE, B, w[0], w[1], w[2], w[3]));
                solve_pde4(R, solver, X, TRACE, B, w, nr, nc, F);
            }
        }
        est = X;
        if (s > 0) {
            float *up = R.planes(L[s - 1].nr, L[s - 1].nc, F);
            DO(R, pdeip_pyr_resize_dev(R.s, X, nr, nc, F, L[s - 1].nr, L[s - 1].nc, 0, up));
            est = up;
        }
    }
    download(R, {{Iout_host, est}}, n0);
}

// What every entry point refuses before it touches the device, first refusal first: a NULL pointer in argument order, the frame
// (check_dims), the term codes where the driver has them (terms: {fstTerm, sndTerm} or null), the merged param.solver, and a
// scl_factor that would not shrink the frame (null: the driver does not check it).
struct Arg {
    const void *p;
    const char *name;
};
#define ARG(p) Arg{p, #p}
int enter(const char *who, std::initializer_list<Arg> pointers, int nrows, int ncols, int frames, const int *terms, int solver, const double *scl_factor)
{
    // the text must stay that of NONNULL (pdeip_ctx.hpp), which names its argument at compile time and so cannot run over a list;
    // tests/test_driver_refusals.py pins it for these entry points
    for (const Arg &a : pointers)
        if (a.p == nullptr) return set_err(PDEIP_ERR_ARG, "%s: argument '%s' is NULL", who, a.name);
    RC(check_dims(who, nrows, ncols, frames));
    if (terms != nullptr) {
        if (terms[0] != PDEIP_TERM_RGB && terms[0] != PDEIP_TERM_GRAD) return set_err(PDEIP_ERR_ARG, "%s: No such fstTerm", who);
        if (terms[1] != PDEIP_TERM_NONE && terms[1] != PDEIP_TERM_RGB && terms[1] != PDEIP_TERM_GRADMAG) return set_err(PDEIP_ERR_ARG, "%s: No such sndTerm", who);
    }
    read_env_once();
    RC(check_solver(who, solver));
    if (scl_factor != nullptr && !(*scl_factor < 1.0)) return set_err(PDEIP_ERR_ARG, "%s: scl_factor must be below 1", who);
    return PDEIP_OK;
}

int tv_entry(const char *who, const float *Iin, int nrows, int ncols, int frames, const pdeip_tv_params *prm, const TvParams &dflt, bool eight, float *Iout)
{
    const TvParams p = merge(prm, dflt);
    RC(enter(who, {ARG(Iin), ARG(Iout)}, nrows, ncols, frames, nullptr, p.solver, &p.scl_factor));
    return play(who, [&](Run &R) { tv_run(R, Iin, nrows, ncols, frames, p, eight, Iout); });
}

// FlowEminND_llin_2D_v10.m:52-67; FlowEminAD_llin_2D_v10.m:52-70 has the same defaults (+ quantile 0.9, diffusion 'image')
const Params FLOW_LLIN_DEFAULTS{0.042, 1.9, 0.01, 1.4843, 0.2915, 0.75, 4, 4, 4, PDEIP_SOLVER_ALR, ALL_SCALES};

} // namespace

extern "C" int pdeip_tvdenoise8(const float *Iin, int nrows, int ncols, int frames, const pdeip_tv_params *prm, float *Iout)
{
    return tv_entry("pdeip_tvdenoise8", Iin, nrows, ncols, frames, prm, TvParams{500.0, 1.75, 0.75, 0.75, 20, 4, PDEIP_SOLVER_ALR}, true, Iout); // TVdenoise8.m:36-44
}

extern "C" int pdeip_tvdenoise4(const float *Iin, int nrows, int ncols, int frames, const pdeip_tv_params *prm, float *Iout)
{
    return tv_entry("pdeip_tvdenoise4", Iin, nrows, ncols, frames, prm, TvParams{5.0, 1.75, 0.5, 0.75, 10, 5, PDEIP_SOLVER_ALR}, false, Iout); // TVdenoise4.m:37-45
}

extern "C" int pdeip_flow_nd_llin(const float *Iin, int nrows, int ncols, int channels, int fst_term, int snd_term, const pdeip_driver_params *prm,
                                  const double *Us, const double *Vs, float *U, float *V)
{
    const char *who = "pdeip_flow_nd_llin";
    const Params p = merge(prm, FLOW_LLIN_DEFAULTS);
    const int terms[2] = {fst_term, snd_term};
    RC(enter(who, {ARG(Iin), ARG(U), ARG(V)}, nrows, ncols, channels, terms, p.solver, &p.scl_factor));
    const Llin d{Iin, nullptr, 2, {Us, Vs}, 20, 2.0, {U, V}};
    return play(who, [&](Run &R) {
        llin_driver(R, d, nrows, ncols, channels, fst_term, snd_term, p,
                    [&](const Level &lv, const Terms &t, Fields &F, double as_diff, bool u_double) { flow_level(R, p, lv, t, F, as_diff, u_double); });
    });
}

extern "C" int pdeip_flow_ad_llin(const float *Iin, int nrows, int ncols, int channels, int fst_term, int snd_term, const pdeip_driver_params *prm,
                                  double quantile, int flow_diffusion, const double *Us, const double *Vs, float *U, float *V)
{
    const char *who = "pdeip_flow_ad_llin";
    const Params p = merge(prm, FLOW_LLIN_DEFAULTS);
    const int terms[2] = {fst_term, snd_term};
    RC(enter(who, {ARG(Iin), ARG(U), ARG(V)}, nrows, ncols, channels, terms, p.solver, &p.scl_factor));
    // deliberately after the shared checks: quantile is an argument of this entry point alone and has always been looked at last
    const double q = or_default(quantile, 0.9);
    if (q > 1.0) return set_err(PDEIP_ERR_ARG, "%s: quantile must be in (0, 1]", who);
    const Llin d{Iin, nullptr, 2, {Us, Vs}, 20, 2.0, {U, V}};
    return play(who, [&](Run &R) {
        llin_driver(R, d, nrows, ncols, channels, fst_term, snd_term, p, [&](const Level &lv, const Terms &t, Fields &F, double as_diff, bool u_double) {
            flow_ad_level(R, p, lv, channels, t, q, flow_diffusion != 0, F, as_diff, u_double);
        });
    });
}

extern "C" int pdeip_disp_nd_llin(const float *Il, const float *Ir, int nrows, int ncols, int channels, int fst_term, int snd_term,
                                  const pdeip_driver_params *prm, const double *Us, float *U)
{
    const char *who = "pdeip_disp_nd_llin";
    const Params p = merge(prm, Params{0.042, 1.9, 0.005, 1.48, 0.29, 0.75, 4, 6, 4, PDEIP_SOLVER_ALR, ALL_SCALES}); // DispEminND_llin_2D.m:51-63
    const int terms[2] = {fst_term, snd_term};
    RC(enter(who, {ARG(Il), ARG(Ir), ARG(U)}, nrows, ncols, channels, terms, p.solver, &p.scl_factor));
    const Llin d{Il, Ir, 1, {Us, nullptr}, 10, 1.75, {U, nullptr}};
    return play(who, [&](Run &R) {
        llin_driver(R, d, nrows, ncols, channels, fst_term, snd_term, p,
                    [&](const Level &lv, const Terms &t, Fields &F, double as_diff, bool u_double) { disp_level(R, p, lv, t, F, as_diff, u_double); });
    });
}

extern "C" int pdeip_flow_hs_elin(const float *Iin, int nrows, int ncols, int channels, const pdeip_driver_params *prm, float *U, float *V)
{
    const char *who = "pdeip_flow_hs_elin";
    // FlowEminHS_elin_2D_v10.m:52-62.  gammaS, firstLoop, secondLoop and scales are not parameters of this driver: the first three
    // are never read, and scales is deliberately put back to "all" whatever the caller's struct holds.
    Params p = merge(prm, Params{0.2, 1.9, 0.0, 0.25, 0.75, 0.75, 1, 1, 20, PDEIP_SOLVER_ALR, ALL_SCALES});
    p.scales = ALL_SCALES;
    RC(enter(who, {ARG(Iin), ARG(U), ARG(V)}, nrows, ncols, channels, nullptr, p.solver, &p.scl_factor));
    return play(who, [&](Run &R) { flow_hs(R, Iin, nrows, ncols, channels, p, U, V); });
}

extern "C" int pdeip_flow_tvl1(const float *Iin, int nrows, int ncols, const pdeip_flow_tvl1_params *prm, float *U, float *V)
{
    const char *who = "pdeip_flow_tvl1";
    Tvl1Params p{15.0, 0.0, 0.25, 0.5, 0.75, 3, 20, ALL_SCALES};
    if (prm != nullptr) {
        p.lambda = or_default(prm->lambda, p.lambda), p.huber = or_default(prm->huber, p.huber), p.tau = or_default(prm->tau, p.tau);
        p.sigma = or_default(prm->sigma, p.sigma), p.scl_factor = or_default(prm->scl_factor, p.scl_factor);
        p.warps = or_default(prm->warps, p.warps), p.iter = or_default(prm->iter, p.iter), p.scales = or_default(prm->scales, p.scales);
    }
    NONNULL(who, Iin); NONNULL(who, U); NONNULL(who, V);
    if (U == V) return set_err(PDEIP_ERR_ARG, "%s: U is V", who);
    if (nrows < 2 || ncols < 2) return set_err(PDEIP_ERR_ARG, "%s: the frames must be at least 2x2 (got %dx%d)", who, nrows, ncols);
    if ((long long)nrows * ncols * 2 > 0x7fffffffLL) return set_err(PDEIP_ERR_ARG, "%s: more than 2^31-1 elements", who);
    RC(tvl1_check_params(who, p.lambda, p.huber, p.iter, p.tau, p.sigma));
    if (!(p.scl_factor < 1.0)) return set_err(PDEIP_ERR_ARG, "%s: scl_factor must be below 1", who);
    if (ncols > 65535) return set_err(PDEIP_ERR_UNSUPPORTED, "%s: more than 65535 columns (got %d): the launch geometry", who, ncols);
    return play(who, [&](Run &R) { flow_tvl1(R, Iin, nrows, ncols, p, U, V); });
}

extern "C" int pdeip_flow_fas_fmg_elin(const float *Iin, int nrows, int ncols, int channels, const pdeip_fas_params *prm, float *U, float *V)
{
    const char *who = "pdeip_flow_fas_fmg_elin";
    const FasParams p = merge(prm, FasParams{0.035, 1.9, 0.03, 0.97, 0.5, 4, 4, PDEIP_SOLVER_ALR, 1, ALL_SCALES}); // FlowEminNDFASFMG_elin_2D_v10.m:53-69
    // deliberately no scl_factor check: this pyramid halves whatever scl_factor says, which only scales restriction and prolongation
    RC(enter(who, {ARG(Iin), ARG(U), ARG(V)}, nrows, ncols, channels, nullptr, p.solver, nullptr));
    return play(who, [&](Run &R) { fas_fmg(R, Iin, nrows, ncols, channels, p, U, V); });
}

extern "C" int pdeip_disp_nd_llin_sym(const float *Il, const float *Ir, int nrows, int ncols, int channels, const pdeip_sym_params *prm, float *U)
{
    const char *who = "pdeip_disp_nd_llin_sym";
    const SymParams p = merge(prm, SymParams{0.035, 0.4, 1.9, 0.25, 0.72, 0.75, 3, 4, 4, PDEIP_SOLVER_ALR}); // DispEminND_llin_sym_2D.m:51-62
    RC(enter(who, {ARG(Il), ARG(Ir), ARG(U)}, nrows, ncols, channels, nullptr, p.solver, &p.scl_factor));
    return play(who, [&](Run &R) { disp_sym(R, Il, Ir, nrows, ncols, channels, p, U); });
}
#undef ARG
