// pdeip_inpaint.hip -- libpdeip.so: a sparse disparity or flow map (NaN = no estimate) made dense again by total-variation inpainting.
//
//   the NaN-aware resize of the pyramid                                        pdeip_nan_resize_dev
//   the starting fill of the coarsest scale                                    pdeip_inpaint_meanfill_dev
//   TRACE / B / the lagged-diffusivity weights of a sparse map, guide optional  pdeip_tv4_inpaint_assemble_dev
//   known pixels get their own bits back                                        pdeip_inpaint_merge_dev
//   the whole run, coarse to fine                                               pdeip_tv_inpaint4(_dev)
//
// Kernels: csrc/pdeip_inpaint.hpp; the contract: include/pdeip.h.  The solver is pdeip_pde_sor4_dev / pdeip_pde_alr4_dev in the
// library's current mode: a pixel whose TRACE is NaN is filled by diffusion from its neighbours (pdeSolvers.c:101-114).
// Nothing is read back in the _dev forms and no launch depends on the data.
//
// Build (build.py): hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -c, one object per translation unit.
#include "pdeip_ctx.hpp"
#include "pdeip_inpaint.hpp"

#include <cmath>
#include <vector>

using namespace pdeip;
using namespace pdeip::inpaint;

namespace {

constexpr int MAX_GRID_Y = 65535; // the column is blockIdx.y

int columns_arg(const char *who, int ncols)
{
    if (ncols > MAX_GRID_Y) return set_err(PDEIP_ERR_UNSUPPORTED, "%s: more than %d columns (got %d)", who, MAX_GRID_Y, ncols);
    return PDEIP_OK;
}

int axis_arg(const char *who, int n_in, int n_out, PyrAxis *A)
{
    *A = pyr_axis_of(n_in, n_out, 0);
    if (A->T > PYR_TMAX) return set_err(PDEIP_ERR_UNSUPPORTED, "%s: shrinking %d -> %d needs %d taps (at most %d)", who, n_in, n_out, A->T, PYR_TMAX);
    return PDEIP_OK;
}

int cover_arg(const char *who, double cover)
{
    if (!(cover > 0.0 && cover <= 1.0)) return set_err(PDEIP_ERR_ARG, "%s: cover must lie in (0, 1] (got %g)", who, cover);
    return PDEIP_OK;
}

int guide_args(const char *who, const void *guide, int guide_channels, int nrows, int ncols, int nframes)
{
    if (guide_channels < 0) return set_err(PDEIP_ERR_ARG, "%s: guide_channels must be >= 0 (got %d)", who, guide_channels);
    if ((guide != nullptr) != (guide_channels > 0))
        return set_err(PDEIP_ERR_ARG, "%s: guide is %s but guide_channels is %d", who, guide ? "given" : "NULL", guide_channels);
    if (guide_channels > 0) RC(check_dims(who, nrows, ncols, nframes + guide_channels));
    return PDEIP_OK;
}

// The driver's parameters with the defaults filled in, and the sizes of its pyramid (finest first).
struct Resolved {
    double alpha, omega, scl_factor, cover, guide_scale;
    int outer_iter, inner_iter, solver, min_size, keep;
    std::vector<int> nr, nc;
};

// Everything refused is refused here, before any HIP call.
int resolve(const char *who, const void *D, int nrows, int ncols, int frames, const void *guide, int guide_channels,
            const pdeip_inpaint_params *u, const void *out, Resolved *p)
{
    NONNULL(who, D);
    NONNULL(who, out);
    RC(check_dims(who, nrows, ncols, frames));
    RC(columns_arg(who, ncols));
    RC(guide_args(who, guide, guide_channels, nrows, ncols, frames));
    *p = Resolved{5.0, 1.75, 0.75, 0.25, 20.0, 10, 5, PDEIP_SOLVER_ALR, 16, 1, {}, {}};
    if (u != nullptr) { // <= 0 or NaN: the default (keep: < 0)
        auto Dd = [](double v, double d) { return (v > 0.0) ? v : d; };
        auto Ii = [](int v, int d) { return v > 0 ? v : d; };
        p->alpha = Dd(u->alpha, p->alpha);
        p->omega = Dd(u->omega, p->omega);
        p->scl_factor = Dd(u->scl_factor, p->scl_factor);
        p->cover = Dd(u->cover, p->cover);
        p->guide_scale = Dd(u->guide_scale, p->guide_scale);
        p->outer_iter = Ii(u->outer_iter, p->outer_iter);
        p->inner_iter = Ii(u->inner_iter, p->inner_iter);
        p->solver = Ii(u->solver, p->solver);
        p->min_size = Ii(u->min_size, p->min_size);
        p->keep = u->keep < 0 ? 1 : (u->keep != 0);
    }
    if (p->solver != PDEIP_SOLVER_SOR && p->solver != PDEIP_SOLVER_ALR)
        return set_err(PDEIP_ERR_ARG, "%s: unknown solver %d (1 point SOR, 2 line relaxation)", who, p->solver);
    if (!(p->scl_factor < 1.0)) return set_err(PDEIP_ERR_ARG, "%s: scl_factor must be below 1 (got %g)", who, p->scl_factor);
    if (!(p->cover <= 1.0)) return set_err(PDEIP_ERR_ARG, "%s: cover must not be above 1 (got %g)", who, p->cover);
    if (!std::isfinite((float)p->alpha) || !std::isfinite((float)p->omega) || !std::isfinite((float)p->guide_scale))
        return set_err(PDEIP_ERR_ARG, "%s: alpha, omega and guide_scale must be finite in single precision", who);
    // level k+1 = ceil(size * scl_factor) while its smaller side is >= min_size (and >= 3, the solvers' smallest frame) and it shrinks
    const int floor_size = p->min_size > 3 ? p->min_size : 3;
    p->nr.push_back(nrows);
    p->nc.push_back(ncols);
    for (;;) {
        const int r = p->nr.back(), c = p->nc.back();
        const int nr = (int)std::ceil(r * p->scl_factor), nc = (int)std::ceil(c * p->scl_factor);
        if ((nr < nc ? nr : nc) < floor_size || (nr == r && nc == c)) break;
        PyrAxis A;
        RC(axis_arg(who, r, nr, &A));
        RC(axis_arg(who, c, nc, &A));
        p->nr.push_back(nr);
        p->nc.push_back(nc);
    }
    return PDEIP_OK;
}

} // namespace

// What pdeip_tv_inpaint4(_dev) would refuse for this frame and these parameters, for a chain that wants to refuse before its first
// launch (pdeip_flow_interpolate): no pointer is dereferenced and no HIP call made.
int pdeip::inpaint_check_params(const char *who, int nrows, int ncols, int frames, const pdeip_inpaint_params *prm)
{
    static const float plane = 0.0f;
    Resolved p;
    return resolve(who, &plane, nrows, ncols, frames, nullptr, 0, prm, &plane, &p);
}

extern "C" int pdeip_nan_resize_dev(void *stream, const float *in, int nrows, int ncols, int nframes, int nrows_out, int ncols_out, double cover,
                                    float *out)
{
    const char *who = "pdeip_nan_resize_dev";
    NONNULL(who, in);
    NONNULL(who, out);
    RC(check_dims(who, nrows, ncols, nframes));
    RC(check_dims(who, nrows_out, ncols_out, nframes));
    RC(columns_arg(who, ncols_out));
    if (nframes > MAX_GRID_Y) return set_err(PDEIP_ERR_UNSUPPORTED, "%s: more than %d frames (got %d)", who, MAX_GRID_Y, nframes);
    if (in == out) return set_err(PDEIP_ERR_ARG, "%s: output must not alias the input", who);
    RC(cover_arg(who, cover));
    PyrAxis R, C;
    RC(axis_arg(who, nrows, nrows_out, &R));
    RC(axis_arg(who, ncols, ncols_out, &C));
    hipLaunchKernelGGL(k_nan_resize, pixel_grid(nrows_out, ncols_out, nframes), dim3(256), 0, static_cast<hipStream_t>(stream), out, in, R, C,
                       nrows, ncols, nrows_out, ncols_out, cover);
    HIPCHK(hipGetLastError());
    tls.last_launches = 1;
    return PDEIP_OK;
}

extern "C" int pdeip_inpaint_meanfill_dev(void *stream, const float *D, int nrows, int ncols, int nframes, float *out)
{
    const char *who = "pdeip_inpaint_meanfill_dev";
    NONNULL(who, D);
    NONNULL(who, out);
    RC(check_dims(who, nrows, ncols, nframes));
    hipLaunchKernelGGL(k_inpaint_meanfill, dim3((unsigned)nframes), dim3(FILL_BLOCK), 0, static_cast<hipStream_t>(stream), out, D, nrows, ncols);
    HIPCHK(hipGetLastError());
    tls.last_launches = 1;
    return PDEIP_OK;
}

extern "C" int pdeip_tv4_inpaint_assemble_dev(void *stream, const float *X, const float *D, const float *guide, int guide_channels,
                                              double guide_scale, int nrows, int ncols, int nframes, float alpha, float *TRACE, float *B,
                                              float *wW, float *wN, float *wE, float *wS)
{
    const char *who = "pdeip_tv4_inpaint_assemble_dev";
    NONNULL(who, X); NONNULL(who, D); NONNULL(who, TRACE); NONNULL(who, B);
    NONNULL(who, wW); NONNULL(who, wN); NONNULL(who, wE); NONNULL(who, wS);
    RC(check_dims(who, nrows, ncols, nframes));
    RC(columns_arg(who, ncols));
    RC(guide_args(who, guide, guide_channels, nrows, ncols, nframes));
    hipLaunchKernelGGL(k_tv4_inpaint_assemble, pixel_grid(nrows, ncols, 1), dim3(256), 0, static_cast<hipStream_t>(stream), TRACE, B, wW, wN, wE,
                       wS, X, D, guide, guide_channels, (float)guide_scale, alpha, nrows, ncols, nframes);
    HIPCHK(hipGetLastError());
    tls.last_launches = 1;
    return PDEIP_OK;
}

static void launch_merge(hipStream_t s, float *out, float *filled, const float *X, const float *D, size_t n)
{
    size_t blocks = (n + FLAT_BLOCK - 1) / FLAT_BLOCK;
    if (blocks > 256 * 16) blocks = 256 * 16; // grid-stride beyond 16 workgroups per compute unit
    hipLaunchKernelGGL(k_inpaint_merge, dim3((unsigned)blocks), dim3(FLAT_BLOCK), 0, s, out, filled, X, D, n);
}

extern "C" int pdeip_inpaint_merge_dev(void *stream, const float *X, const float *D, int nrows, int ncols, int nframes, float *out,
                                       float *filled_out)
{
    const char *who = "pdeip_inpaint_merge_dev";
    NONNULL(who, X);
    NONNULL(who, D);
    NONNULL(who, out);
    RC(check_dims(who, nrows, ncols, nframes));
    launch_merge(static_cast<hipStream_t>(stream), out, filled_out, X, D, (size_t)nrows * ncols * nframes);
    HIPCHK(hipGetLastError());
    tls.last_launches = 1;
    return PDEIP_OK;
}

// The run.  Workspace (WS_DRIVER), in floats, every block padded to 4: per coarser level k >= 1 the map D_k [nr_k x nc_k x frames] and
// the guide G_k [nr_k x nc_k x guide_channels] (level 0 is the caller's own planes); then eight blocks of the finest level's
// [nrows x ncols x frames], shared by all levels: the estimate and its resized twin, TRACE, B and the four weight planes.
extern "C" int pdeip_tv_inpaint4_dev(void *stream, const float *D, int nrows, int ncols, int frames, const float *guide, int guide_channels,
                                     const pdeip_inpaint_params *prm, float *out, float *filled_out)
{
    const char *who = "pdeip_tv_inpaint4_dev";
    Resolved p;
    RC(resolve(who, D, nrows, ncols, frames, guide, guide_channels, prm, out, &p));
    read_env_once();
    const int mode = g.mode;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int K = (int)p.nr.size(), F = frames, G = guide_channels;
    const size_t full = pad4((size_t)nrows * ncols * F);
    size_t total = 8 * full;
    for (int k = 1; k < K; k++) total += pad4((size_t)p.nr[k] * p.nc[k] * F) + pad4((size_t)p.nr[k] * p.nc[k] * G);
    float *ws = nullptr;
    RC(ws_get(WS_DRIVER, total * sizeof(float), &ws));
    float *Xa = ws, *Xb = Xa + full, *TRACE = Xb + full, *B = TRACE + full, *w[4];
    for (int k = 0; k < 4; k++) w[k] = B + (size_t)(k + 1) * full;
    std::vector<const float *> Dk(K), Gk(K);
    Dk[0] = D;
    Gk[0] = guide;
    float *next = w[3] + full;
    int launches = 0;
    for (int k = 1; k < K; k++) {
        float *d = next, *gd = d + pad4((size_t)p.nr[k] * p.nc[k] * F);
        next = gd + pad4((size_t)p.nr[k] * p.nc[k] * G);
        RC(pdeip_nan_resize_dev(s, Dk[k - 1], p.nr[k - 1], p.nc[k - 1], F, p.nr[k], p.nc[k], p.cover, d));
        launches++;
        if (G > 0) {
            RC(pdeip_pyr_resize_dev(s, Gk[k - 1], p.nr[k - 1], p.nc[k - 1], G, p.nr[k], p.nc[k], 0, gd));
            launches++;
        }
        Dk[k] = d;
        Gk[k] = G > 0 ? gd : nullptr;
    }
    float *X = Xa, *Xo = Xb;
    RC(pdeip_inpaint_meanfill_dev(s, Dk[K - 1], p.nr[K - 1], p.nc[K - 1], F, X));
    launches++;
    for (int k = K - 1; k >= 0; k--) {
        const int nr = p.nr[k], nc = p.nc[k];
        for (int it = 0; it <= p.outer_iter; it++) {
            RC(pdeip_tv4_inpaint_assemble_dev(s, X, Dk[k], Gk[k], G, p.guide_scale, nr, nc, F, (float)p.alpha, TRACE, B, w[0], w[1], w[2], w[3]));
            launches++;
            if (p.solver == PDEIP_SOLVER_SOR) RC(pdeip_pde_sor4_dev(s, X, TRACE, B, w[0], w[1], w[2], w[3], nr, nc, F, p.inner_iter, (float)p.omega, mode, 0));
            else RC(pdeip_pde_alr4_dev(s, X, TRACE, B, w[0], w[1], w[2], w[3], nr, nc, F, p.inner_iter, (float)p.omega, mode));
            launches += tls.last_launches;
        }
        if (k > 0) {
            RC(pdeip_pyr_resize_dev(s, X, nr, nc, F, p.nr[k - 1], p.nc[k - 1], 0, Xo));
            launches++;
            float *t = X;
            X = Xo;
            Xo = t;
        }
    }
    const size_t n = (size_t)nrows * ncols * F;
    if (p.keep) {
        launch_merge(s, out, filled_out, X, D, n);
        launches++;
    } else {
        RC(copy_d2d(s, out, X, n));
        launches++;
        if (filled_out != nullptr) {
            launch_merge(s, nullptr, filled_out, X, D, n);
            launches++;
        }
    }
    HIPCHK(hipGetLastError());
    tls.last_launches = launches;
    return PDEIP_OK;
}

extern "C" int pdeip_tv_inpaint4(const float *D, int nrows, int ncols, int frames, const float *guide, int guide_channels,
                                 const pdeip_inpaint_params *prm, float *out, float *filled_out)
{
    const char *who = "pdeip_tv_inpaint4";
    Resolved p;
    RC(resolve(who, D, nrows, ncols, frames, guide, guide_channels, prm, out, &p));
    RC(use_device());
    const size_t n = (size_t)nrows * ncols, nd = pad4(n * frames), ng = pad4(n * guide_channels);
    // arena: D, out, filled, guide
    float *ar = nullptr;
    RC(ws_get(WS_ARENA, (3 * nd + ng) * sizeof(float), &ar));
    float *dD = ar, *dout = dD + nd, *dfilled = filled_out ? dout + nd : nullptr, *dguide = guide_channels > 0 ? dout + 2 * nd : nullptr;
    HIPCHK(hipMemcpy(dD, D, n * frames * sizeof(float), hipMemcpyHostToDevice));
    if (dguide) HIPCHK(hipMemcpy(dguide, guide, n * guide_channels * sizeof(float), hipMemcpyHostToDevice));
    RC(pdeip_tv_inpaint4_dev(nullptr, dD, nrows, ncols, frames, dguide, guide_channels, prm, dout, dfilled));
    HIPCHK(hipMemcpy(out, dout, n * frames * sizeof(float), hipMemcpyDeviceToHost));
    if (filled_out) HIPCHK(hipMemcpy(filled_out, dfilled, n * frames * sizeof(float), hipMemcpyDeviceToHost));
    RC(pdeip_persist_error());
    return PDEIP_OK;
}
