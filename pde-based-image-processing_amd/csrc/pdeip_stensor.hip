// pdeip_stensor.hip -- libpdeip.so: structure-tensor anisotropic diffusion.  pdeip_gauss(_dev) smooths at a chosen scale,
// pdeip_structure_tensor_dev and pdeip_st_weights_dev are the stages of one semi-implicit step, and pdeip_diffusion8(_dev) is the
// resident filter: Weickert's edge-enhancing (EED) and coherence-enhancing (CED) diffusion, each step one PDEsolver8 solve by the
// library's own 9-point solvers (pdeip_pde_sor8_dev / pdeip_pde_alr8_dev) in the library's current ordering.
//
// Kernels: csrc/pdeip_stensor.hpp; the 8-weight assembly is pdeip_tensor8.hpp's, shared with TVdenoise8.
//
// Build (build.py): hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -c, one object per translation unit.
#include "pdeip_ctx.hpp"
#include "pdeip_stensor.hpp"

#include <cmath>

using namespace pdeip;
using namespace pdeip::st;

namespace {

constexpr int MAX_GRID_YZ = 65535; // the column (or a block of columns) is blockIdx.y, the frame blockIdx.z

// R = ceil(3 sigma) and the 2R + 1 normalised taps; everything refused is refused without a HIP call.
int taps_of(const char *who, const char *name, double sigma, GaussTaps *T)
{
    if (!std::isfinite(sigma) || sigma < 0.0) return set_err(PDEIP_ERR_ARG, "%s: %s must be finite and >= 0 (got %g)", who, name, sigma);
    // ceil of the exact product: where the double 3 sigma rounds down onto an integer the radius is the next one (the smallest sigma
    // above 32 / 3 gives the double 32.0 and needs 33 taps)
    const double p3 = 3.0 * sigma;
    double r = std::ceil(p3);
    if (r == p3 && std::fma(3.0, sigma, -p3) > 0.0) r += 1.0;
    if (r > (double)GAUSS_RMAX)
        return set_err(PDEIP_ERR_UNSUPPORTED, "%s: %s = %g needs a radius of %.0f taps (at most %d)", who, name, sigma, r, GAUSS_RMAX);
    const int R = (int)r;
    double g[2 * GAUSS_RMAX + 1], sum = 0.0;
    for (int k = -R; k <= R; k++) {
        g[k + R] = k == 0 ? 1.0 : std::exp(-(double)(k * k) / (2.0 * sigma * sigma)); // (a sigma whose square underflows: the centre tap alone)
        sum += g[k + R];
    }
    for (int k = 0; k <= 2 * R; k++) T->g[k] = (float)(g[k] / sum);
    T->R = R;
    return PDEIP_OK;
}

int plane_dims(const char *who, int nrows, int ncols, int frames)
{
    RC(check_dims(who, nrows, ncols, frames));
    if (ncols > MAX_GRID_YZ) return set_err(PDEIP_ERR_UNSUPPORTED, "%s: more than %d columns (got %d)", who, MAX_GRID_YZ, ncols);
    if (frames > MAX_GRID_YZ) return set_err(PDEIP_ERR_UNSUPPORTED, "%s: more than %d frames (got %d)", who, MAX_GRID_YZ, frames);
    return PDEIP_OK;
}

// The two passes of one smoothing, T.R > 0: rows into `mid`, columns into `out`.
int gauss_passes(hipStream_t s, const float *in, int nrows, int ncols, int frames, const GaussTaps &T, float *mid, float *out)
{
    const unsigned rt = (unsigned)((nrows + GAUSS_T - 1) / GAUSS_T);
    const dim3 block(GAUSS_T, GAUSS_WAVES);
    hipLaunchKernelGGL(k_gauss_rows, dim3(rt, (unsigned)((ncols + GAUSS_WAVES - 1) / GAUSS_WAVES), (unsigned)frames), block, 0, s, mid, in, T, nrows, ncols);
    hipLaunchKernelGGL(k_gauss_cols, dim3(rt, (unsigned)((ncols + GAUSS_T - 1) / GAUSS_T), (unsigned)frames), block,
                       (size_t)(GAUSS_T + 2 * T.R) * GAUSS_T * sizeof(float), s, out, mid, T, nrows, ncols);
    HIPCHK(hipGetLastError());
    return PDEIP_OK;
}

// What a parameter struct resolves to.  NaN members (or no struct) take the defaults of the mode: CED sigma 0.7, rho 4, alpha
// 0.001, C 1; EED sigma 1.5, rho 0, lambda 6; both tau 1, 10 iterations, point SOR with 4 sweeps at omega 1.
struct Resolved {
    TensorRule rule;
    double sigma, rho, tau, omega;
    int iters, inner_iter, solver;
    GaussTaps gs, gr;
};

int resolve_rule(const char *who, const pdeip_diffusion8_params *u, TensorRule *rule)
{
    auto pick = [](double v, double d) { return std::isnan(v) ? d : v; };
    const double mode = u ? pick(u->mode, 1.0) : 1.0;
    if (mode != 0.0 && mode != 1.0) return set_err(PDEIP_ERR_ARG, "%s: mode must be 0 (EED) or 1 (CED) (got %g)", who, mode);
    rule->ced = mode == 1.0;
    rule->lambda = u ? pick(u->lambda, 6.0) : 6.0;
    rule->alpha = u ? pick(u->alpha, 0.001) : 0.001;
    rule->C = u ? pick(u->C, 1.0) : 1.0;
    if (!rule->ced && !(std::isfinite(rule->lambda) && rule->lambda > 0.0))
        return set_err(PDEIP_ERR_ARG, "%s: lambda must be finite and > 0 (got %g)", who, rule->lambda);
    if (rule->ced && !(rule->alpha >= 0.0 && rule->alpha <= 1.0)) return set_err(PDEIP_ERR_ARG, "%s: alpha must lie in [0, 1] (got %g)", who, rule->alpha);
    if (rule->ced && !(std::isfinite(rule->C) && rule->C > 0.0)) return set_err(PDEIP_ERR_ARG, "%s: C must be finite and > 0 (got %g)", who, rule->C);
    return PDEIP_OK;
}

int check_tau(const char *who, double tau)
{
    if (!std::isfinite(tau) || tau < 0.0) return set_err(PDEIP_ERR_ARG, "%s: tau must be finite and >= 0 (got %g)", who, tau);
    return PDEIP_OK;
}

// floor of a count given as a double: negative counts none, an infinite or over-large one is refused
int count_of(const char *who, const char *name, double v, int *out)
{
    if (std::isinf(v)) return set_err(PDEIP_ERR_ARG, "%s: %s must be finite (got %g)", who, name, v);
    if (v > 2147483646.0) return set_err(PDEIP_ERR_ARG, "%s: %s = %g is too large", who, name, v);
    *out = v >= 0.0 ? (int)std::floor(v) : 0;
    return PDEIP_OK;
}

// The driver's workspace in floats: J (3 planes of the image), then planes of the image inside its one-pixel ring: TRACE, the eight
// weights, and the iterate and B of every channel.
size_t padded(int nrows, int ncols) { return pad4((size_t)(nrows + 2) * (ncols + 2)); }
size_t step_floats(int nrows, int ncols, int channels) { return 3 * pad4((size_t)nrows * ncols) + (9 + 2 * (size_t)channels) * padded(nrows, ncols); }

int resolve(const char *who, int nrows, int ncols, int channels, const pdeip_diffusion8_params *u, Resolved *p)
{
    RC(plane_dims(who, nrows, ncols, channels));
    RC(resolve_rule(who, u, &p->rule));
    auto pick = [](double v, double d) { return std::isnan(v) ? d : v; };
    p->sigma = u ? pick(u->sigma, p->rule.ced ? 0.7 : 1.5) : (p->rule.ced ? 0.7 : 1.5);
    p->rho = u ? pick(u->rho, p->rule.ced ? 4.0 : 0.0) : (p->rule.ced ? 4.0 : 0.0);
    p->tau = u ? pick(u->tau, 1.0) : 1.0;
    p->omega = u ? pick(u->omega, 1.0) : 1.0;
    const double solver = u ? pick(u->solver, 1.0) : 1.0;
    RC(taps_of(who, "sigma", p->sigma, &p->gs));
    RC(taps_of(who, "rho", p->rho, &p->gr));
    RC(check_tau(who, p->tau));
    if (!std::isfinite((float)p->omega)) return set_err(PDEIP_ERR_ARG, "%s: omega must be finite in single precision (got %g)", who, p->omega);
    if (solver != (double)PDEIP_SOLVER_SOR && solver != (double)PDEIP_SOLVER_ALR) return check_solver(who, -1);
    p->solver = (int)solver;
    RC(count_of(who, "iters", u ? pick(u->iters, 10.0) : 10.0, &p->iters));
    RC(count_of(who, "inner_iter", u ? pick(u->inner_iter, 4.0) : 4.0, &p->inner_iter));
    if (ncols + 2 > MAX_GRID_YZ) return set_err(PDEIP_ERR_UNSUPPORTED, "%s: more than %d columns (got %d)", who, MAX_GRID_YZ - 2, ncols);
    if (step_floats(nrows, ncols, channels) > (size_t)0x7fffffff)
        return set_err(PDEIP_ERR_ARG, "%s: a workspace of more than 2^31-1 elements (%zu)", who, step_floats(nrows, ncols, channels));
    return PDEIP_OK;
}

// J of I with the taps already made.  Workspace (WS_STENSOR): v = G_sigma * I [nrows x ncols x channels], then the three product
// planes when they are smoothed; the smoothing's own intermediate plane is WS_GAUSS.  sigma = 0 reads I itself and rho = 0 writes the
// products to J, so the call is 2 [sigma > 0] + 1 + 2 [rho > 0] launches.
int structure_tensor(hipStream_t s, const float *I, int nrows, int ncols, int channels, const GaussTaps &gs, const GaussTaps &gr, float *J, int *launches)
{
    const size_t n = (size_t)nrows * ncols, pc = pad4(n * channels), pn = pad4(n);
    const int most = channels > 3 ? channels : 3;
    float *ws = nullptr, *mid = nullptr;
    if (gs.R > 0 || gr.R > 0) {
        RC(ws_get(WS_STENSOR, (pc + 3 * pn) * sizeof(float), &ws));
        RC(ws_get(WS_GAUSS, pad4(n * most) * sizeof(float), &mid));
    }
    const float *V = I;
    *launches = 1;
    if (gs.R > 0) {
        RC(gauss_passes(s, I, nrows, ncols, channels, gs, mid, ws));
        V = ws;
        *launches += 2;
    }
    float *P = gr.R > 0 ? ws + pc : J; // three consecutive planes either way
    const double a = 4.0 + std::sqrt(8.0);
    hipLaunchKernelGGL(k_st_products, pixel_grid(nrows, ncols, 1), dim3(256), 0, s, P, P + n, P + 2 * n, V, nrows, ncols, channels,
                       (float)(1.0 / a), (float)(std::sqrt(2.0) / a));
    HIPCHK(hipGetLastError());
    if (gr.R > 0) {
        RC(gauss_passes(s, P, nrows, ncols, 3, gr, mid, J));
        *launches += 2;
    }
    return PDEIP_OK;
}

int st_weights(hipStream_t s, const float *J, int nrows, int ncols, const TensorRule &rule, double tau, float *TRACE, float *w8, int pad)
{
    const size_t n = (size_t)nrows * ncols;
    hipLaunchKernelGGL(k_st_weights, dim3((unsigned)((nrows + TT_R - 1) / TT_R), (unsigned)((ncols + TT_C - 1) / TT_C)), dim3(TT_R, TT_C), 0, s, TRACE, w8, J,
                       J + n, J + 2 * n, rule, tau, nrows, ncols, pad);
    HIPCHK(hipGetLastError());
    return PDEIP_OK;
}

int weights_entry(const char *who, void *stream, const float *J, int nrows, int ncols, const pdeip_diffusion8_params *prm, double tau, float *TRACE,
                  float *w8, int pad)
{
    NONNULL(who, J); NONNULL(who, TRACE); NONNULL(who, w8);
    RC(plane_dims(who, nrows, ncols, 1));
    TensorRule rule;
    RC(resolve_rule(who, prm, &rule));
    RC(check_tau(who, tau));
    RC(st_weights(static_cast<hipStream_t>(stream), J, nrows, ncols, rule, tau, TRACE, w8, pad));
    tls.last_launches = 1;
    return PDEIP_OK;
}

int st_pad(hipStream_t s, const float *in, int nrows, int ncols, int frames, float *out, float *out2)
{
    hipLaunchKernelGGL(k_st_pad, pixel_grid(nrows + 2, ncols + 2, frames), dim3(256), 0, s, out, out2, in, nrows, ncols);
    HIPCHK(hipGetLastError());
    return PDEIP_OK;
}

int st_crop(hipStream_t s, const float *in, int nrows, int ncols, int frames, float *out)
{
    hipLaunchKernelGGL(k_st_crop, pixel_grid(nrows, ncols, frames), dim3(256), 0, s, out, in, nrows, ncols);
    HIPCHK(hipGetLastError());
    return PDEIP_OK;
}

int pad_dims(const char *who, int nrows, int ncols, int frames)
{
    RC(plane_dims(who, nrows, ncols, frames));
    if (ncols + 2 > MAX_GRID_YZ) return set_err(PDEIP_ERR_UNSUPPORTED, "%s: more than %d columns (got %d)", who, MAX_GRID_YZ - 2, ncols);
    if ((long long)(nrows + 2) * (ncols + 2) * frames > 0x7fffffffLL) return set_err(PDEIP_ERR_ARG, "%s: more than 2^31-1 elements with the ring", who);
    return PDEIP_OK;
}

} // namespace

extern "C" int pdeip_gauss_taps(double sigma, float *taps, int capacity, int *radius)
{
    const char *who = "pdeip_gauss_taps";
    NONNULL(who, taps); NONNULL(who, radius);
    GaussTaps T;
    RC(taps_of(who, "sigma", sigma, &T));
    if (capacity < 2 * T.R + 1) return set_err(PDEIP_ERR_ARG, "%s: capacity %d is below the %d taps of sigma = %g", who, capacity, 2 * T.R + 1, sigma);
    for (int k = 0; k <= 2 * T.R; k++) taps[k] = T.g[k];
    *radius = T.R;
    return PDEIP_OK;
}

extern "C" int pdeip_gauss_dev(void *stream, const float *in, int nrows, int ncols, int frames, double sigma, float *out)
{
    const char *who = "pdeip_gauss_dev";
    NONNULL(who, in); NONNULL(who, out);
    RC(plane_dims(who, nrows, ncols, frames));
    GaussTaps T;
    RC(taps_of(who, "sigma", sigma, &T));
    if (in == out) return set_err(PDEIP_ERR_ARG, "%s: output aliases the input", who);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t nf = (size_t)nrows * ncols * frames;
    if (T.R == 0) {
        RC(copy_d2d(s, out, in, nf));
        tls.last_launches = 1;
        return PDEIP_OK;
    }
    float *mid = nullptr;
    RC(ws_get(WS_GAUSS, pad4(nf) * sizeof(float), &mid));
    RC(gauss_passes(s, in, nrows, ncols, frames, T, mid, out));
    tls.last_launches = 2;
    return PDEIP_OK;
}

extern "C" int pdeip_gauss(const float *in, int nrows, int ncols, int frames, double sigma, float *out)
{
    const char *who = "pdeip_gauss";
    NONNULL(who, in); NONNULL(who, out);
    RC(plane_dims(who, nrows, ncols, frames));
    GaussTaps T;
    RC(taps_of(who, "sigma", sigma, &T));
    if (in == out) return set_err(PDEIP_ERR_ARG, "%s: output aliases the input", who);
    RC(use_device());
    const size_t nf = (size_t)nrows * ncols * frames;
    float *ar = nullptr;
    RC(ws_get(WS_ARENA, 2 * pad4(nf) * sizeof(float), &ar));
    HIPCHK(hipMemcpy(ar, in, nf * sizeof(float), hipMemcpyHostToDevice));
    RC(pdeip_gauss_dev(nullptr, ar, nrows, ncols, frames, sigma, ar + pad4(nf)));
    HIPCHK(hipMemcpy(out, ar + pad4(nf), nf * sizeof(float), hipMemcpyDeviceToHost));
    return PDEIP_OK;
}

extern "C" int pdeip_structure_tensor_dev(void *stream, const float *I, int nrows, int ncols, int channels, double sigma, double rho, float *J)
{
    const char *who = "pdeip_structure_tensor_dev";
    NONNULL(who, I); NONNULL(who, J);
    RC(plane_dims(who, nrows, ncols, channels));
    GaussTaps gs, gr;
    RC(taps_of(who, "sigma", sigma, &gs));
    RC(taps_of(who, "rho", rho, &gr));
    if (I == J) return set_err(PDEIP_ERR_ARG, "%s: J aliases the image", who);
    int launches = 0;
    RC(structure_tensor(static_cast<hipStream_t>(stream), I, nrows, ncols, channels, gs, gr, J, &launches));
    tls.last_launches = launches;
    return PDEIP_OK;
}

extern "C" int pdeip_st_weights_dev(void *stream, const float *J, int nrows, int ncols, const pdeip_diffusion8_params *prm, double tau, float *TRACE,
                                    float *w8)
{
    return weights_entry("pdeip_st_weights_dev", stream, J, nrows, ncols, prm, tau, TRACE, w8, 0);
}

extern "C" int pdeip_st_weights_padded_dev(void *stream, const float *J, int nrows, int ncols, const pdeip_diffusion8_params *prm, double tau,
                                           float *TRACE, float *w8)
{
    const char *who = "pdeip_st_weights_padded_dev";
    RC(pad_dims(who, nrows, ncols, 8));
    return weights_entry(who, stream, J, nrows, ncols, prm, tau, TRACE, w8, 1);
}

extern "C" int pdeip_st_pad_dev(void *stream, const float *in, int nrows, int ncols, int frames, float *out, float *out2)
{
    const char *who = "pdeip_st_pad_dev";
    NONNULL(who, in); NONNULL(who, out);
    RC(pad_dims(who, nrows, ncols, frames));
    if (in == out || in == out2) return set_err(PDEIP_ERR_ARG, "%s: output aliases the input", who);
    RC(st_pad(static_cast<hipStream_t>(stream), in, nrows, ncols, frames, out, out2));
    tls.last_launches = 1;
    return PDEIP_OK;
}

extern "C" int pdeip_st_crop_dev(void *stream, const float *in, int nrows, int ncols, int frames, float *out)
{
    const char *who = "pdeip_st_crop_dev";
    NONNULL(who, in); NONNULL(who, out);
    RC(pad_dims(who, nrows, ncols, frames));
    if (in == out) return set_err(PDEIP_ERR_ARG, "%s: output aliases the input", who);
    RC(st_crop(static_cast<hipStream_t>(stream), in, nrows, ncols, frames, out));
    tls.last_launches = 1;
    return PDEIP_OK;
}

// The run: Iout = Iin, then per iteration J of Iout, the weights and TRACE inside their ring, every channel of Iout inside its ring
// as the iterate and as B (one launch), per channel one solver call in place on the ringed iterate -- all channels on the one set
// of weight planes --, and the insides back to Iout.  Workspace (WS_DRIVER): step_floats().
extern "C" int pdeip_diffusion8_dev(void *stream, const float *Iin, int nrows, int ncols, int channels, const pdeip_diffusion8_params *prm, float *Iout)
{
    const char *who = "pdeip_diffusion8_dev";
    NONNULL(who, Iin); NONNULL(who, Iout);
    Resolved p;
    RC(resolve(who, nrows, ncols, channels, prm, &p));
    read_env_once();
    const int mode = g.mode;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t n = (size_t)nrows * ncols, np = (size_t)(nrows + 2) * (ncols + 2);
    int launches = 0;
    if (Iout != Iin) {
        RC(copy_d2d(s, Iout, Iin, n * channels));
        launches++;
    }
    if (p.iters > 0) {
        float *ws = nullptr;
        RC(ws_get(WS_DRIVER, step_floats(nrows, ncols, channels) * sizeof(float), &ws));
        float *J = ws, *TRACE = J + 3 * pad4(n), *w = TRACE + padded(nrows, ncols), *X = w + 8 * padded(nrows, ncols), *B = X + channels * padded(nrows, ncols);
        for (int it = 0; it < p.iters; it++) {
            int part = 0;
            RC(structure_tensor(s, Iout, nrows, ncols, channels, p.gs, p.gr, J, &part));
            RC(st_weights(s, J, nrows, ncols, p.rule, p.tau, TRACE, w, 1));
            RC(st_pad(s, Iout, nrows, ncols, channels, X, B));
            launches += part + 2;
            for (int c = 0; c < channels; c++) {
                float *x = X + c * np, *b = B + c * np;
                if (p.solver == PDEIP_SOLVER_SOR)
                    RC(pdeip_pde_sor8_dev(s, x, TRACE, b, w, w + np, w + 2 * np, w + 3 * np, w + 4 * np, w + 5 * np, w + 6 * np, w + 7 * np, nrows + 2, ncols + 2, 1,
                                          p.inner_iter, (float)p.omega, mode, 0));
                else
                    RC(pdeip_pde_alr8_dev(s, x, TRACE, b, w, w + np, w + 2 * np, w + 3 * np, w + 4 * np, w + 5 * np, w + 6 * np, w + 7 * np, nrows + 2, ncols + 2, 1,
                                          p.inner_iter, (float)p.omega, mode));
                launches += tls.last_launches;
            }
            RC(st_crop(s, X, nrows, ncols, channels, Iout));
            launches++;
        }
    }
    tls.last_launches = launches;
    return PDEIP_OK;
}

extern "C" int pdeip_diffusion8(const float *Iin, int nrows, int ncols, int channels, const pdeip_diffusion8_params *prm, float *Iout)
{
    const char *who = "pdeip_diffusion8";
    NONNULL(who, Iin); NONNULL(who, Iout);
    Resolved p;
    RC(resolve(who, nrows, ncols, channels, prm, &p));
    RC(use_device());
    const size_t nc = (size_t)nrows * ncols * channels;
    float *dI = nullptr;
    RC(ws_get(WS_ARENA, pad4(nc) * sizeof(float), &dI));
    HIPCHK(hipMemcpy(dI, Iin, nc * sizeof(float), hipMemcpyHostToDevice));
    RC(pdeip_diffusion8_dev(nullptr, dI, nrows, ncols, channels, prm, dI));
    HIPCHK(hipMemcpy(Iout, dI, nc * sizeof(float), hipMemcpyDeviceToHost));
    RC(pdeip_persist_error());
    return PDEIP_OK;
}
