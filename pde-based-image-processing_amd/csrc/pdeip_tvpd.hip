// pdeip_tvpd.hip -- libpdeip.so: primal-dual total variation, TV-L1 / ROF / Huber-TV (pdeip_tv_pd, pdeip_tv_pd_dev).
//
// Kernels: csrc/pdeip_tvpd.hpp; the contract: include/pdeip.h.  The call has no ordering, so pdeip_set_mode does not apply.  Nothing is
// read back in the _dev form and no launch depends on the data.
//
// Launches of a call with iter iterations in blocks of T (T = 1: single steps), as pdeip_last_launch_count() reports them:
//   [3 with u0 == NULL: pdeip_nearest_fill_dev]  +  iter / T blocked launches  +  iter % T single steps  [T > 1]
//   iter == 0: the start alone, 3 launches with u0 == NULL (the fill goes straight to u_out), 1 copy otherwise.
// PDEIP_TVPD_STEPS: unset or 0 the library's choice (DEFAULT_T), 1 single steps, 2 / 4 / 8 that block.
//
// Build (build.py): hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -c, one object per translation unit.
#include "pdeip_ctx.hpp"
#include "pdeip_tvpd.hpp"

#include <cmath>

using namespace pdeip;
using namespace pdeip::tvpd;

namespace {

constexpr int DEFAULT_T = 4;
constexpr int MAX_GRID_YZ = 65535;

struct Plan {
    Consts c;
    int iter, T;
};

// Everything refused is refused here, before any HIP call.
int tvpd_args(const char *who, const float *f, const float *u0, int nrows, int ncols, int frames, const pdeip_tvpd_params *prm, const float *u_out,
              Plan *plan)
{
    NONNULL(who, f); NONNULL(who, u_out); NONNULL(who, prm);
    if (u_out == f || u_out == u0) return set_err(PDEIP_ERR_ARG, "%s: u_out is f or u0", who);
    if (frames < 1) return set_err(PDEIP_ERR_ARG, "%s: frames must be >= 1 (got %d)", who, frames);
    if (nrows < 1 || ncols < 1) return set_err(PDEIP_ERR_ARG, "%s: the plane must be at least 1x1 (got %dx%d)", who, nrows, ncols);
    if ((long long)nrows * ncols * frames > 0x7fffffffLL) return set_err(PDEIP_ERR_ARG, "%s: more than 2^31-1 elements", who);
    if (prm->model != PDEIP_TVPD_L1 && prm->model != PDEIP_TVPD_L2)
        return set_err(PDEIP_ERR_ARG, "%s: unknown model %d (PDEIP_TVPD_L1, PDEIP_TVPD_L2)", who, prm->model);
    if (!(prm->lambda >= 0.0) || !std::isfinite(prm->lambda)) return set_err(PDEIP_ERR_ARG, "%s: lambda must be finite and >= 0 (got %g)", who, prm->lambda);
    if (!(prm->huber >= 0.0) || !std::isfinite(prm->huber)) return set_err(PDEIP_ERR_ARG, "%s: huber must be finite and >= 0 (got %g)", who, prm->huber);
    if (prm->iter < 0) return set_err(PDEIP_ERR_ARG, "%s: iter must be >= 0 (got %d)", who, prm->iter);
    const double tau = std::isnan(prm->tau) ? 0.25 : prm->tau, sigma = std::isnan(prm->sigma) ? 0.5 : prm->sigma;
    if (!(tau > 0.0) || !std::isfinite(tau)) return set_err(PDEIP_ERR_ARG, "%s: tau must be positive and finite (got %g)", who, tau);
    if (!(sigma > 0.0) || !std::isfinite(sigma)) return set_err(PDEIP_ERR_ARG, "%s: sigma must be positive and finite (got %g)", who, sigma);
    if (tau * sigma * 8.0 > 1.0) return set_err(PDEIP_ERR_ARG, "%s: tau * sigma * 8 must not exceed 1 (got %g)", who, tau * sigma * 8.0);
    if (ncols > MAX_GRID_YZ || frames > MAX_GRID_YZ)
        return set_err(PDEIP_ERR_UNSUPPORTED, "%s: more than %d columns or frames (got %d, %d): the launch geometry", who, MAX_GRID_YZ, ncols, frames);
    const int steps = env_int("PDEIP_TVPD_STEPS", 0);
    if (steps != 0 && steps != 1 && steps != 2 && steps != 4 && steps != 8)
        return set_err(PDEIP_ERR_ARG, "%s: PDEIP_TVPD_STEPS=%d is not a supported block (0, 1, 2, 4, 8)", who, steps);
    // the constants, each formed once in float32
    const float tau_f = (float)tau, sigma_f = (float)sigma, lambda_f = (float)prm->lambda, huber_f = (float)prm->huber;
    Consts &c = plan->c;
    c.sigma = sigma_f;
    c.tau = tau_f;
    c.tl = tau_f * lambda_f;
    c.onep_tl = 1.0f + c.tl;
    const float sh = sigma_f * huber_f;
    c.hub_den = 1.0f + sh;
    c.l2 = prm->model == PDEIP_TVPD_L2;
    c.huber = huber_f > 0.0f;
    plan->iter = prm->iter;
    plan->T = steps == 0 ? DEFAULT_T : steps;
    return PDEIP_OK;
}

template <int T>
int launch_block(hipStream_t s, const float *U, const float *UP, const float *PX, const float *PY, const float *F, int nrows, int ncols, int frames,
                 const Consts &c, float *Uo, float *UPo, float *PXo, float *PYo)
{
    const size_t lds = block_lds_bytes<T>();
    RC(ensure_lds(reinterpret_cast<const void *>(&k_tvpd_block<T>), lds));
    const dim3 grid((unsigned)((nrows + TILE_R - 1) / TILE_R), (unsigned)((ncols + TILE_C - 1) / TILE_C), (unsigned)frames);
    hipLaunchKernelGGL(k_tvpd_block<T>, grid, dim3(BLOCK), lds, s, U, UP, PX, PY, F, nrows, ncols, c, Uo, UPo, PXo, PYo);
    return PDEIP_OK;
}

// The iterations on s from the start `start` (never written).  ws: 8 planes of pad4(N) floats -- four of u, two of px, two of py.
int run_tvpd(hipStream_t s, const float *f, const float *start, int nrows, int ncols, int frames, const Plan &plan, float *ws, float *u_out,
             int *launches)
{
    const size_t pN = pad4((size_t)nrows * ncols * frames);
    float *Ub[4] = {ws, ws + pN, ws + 2 * pN, ws + 3 * pN};
    float *PXb[2] = {ws + 4 * pN, ws + 5 * pN}, *PYb[2] = {ws + 6 * pN, ws + 7 * pN};
    const float *u = start, *up = start;
    int pcur = -1; // the buffer that holds p; -1: p is zero
    const auto free_u = [&](const float *not_this) {
        for (float *b : Ub)
            if (b != u && b != up && b != not_this) return b;
        return (float *)nullptr; // not reached: four buffers, three excluded
    };
    const int nblock = plan.T > 1 ? plan.iter / plan.T : 0, nstep = plan.iter - nblock * plan.T, total = nblock + nstep;
    for (int l = 0; l < total; l++) {
        const bool last = l == total - 1;
        const int pnew = pcur == 0 ? 1 : 0;
        const float *px = pcur < 0 ? nullptr : PXb[pcur], *py = pcur < 0 ? nullptr : PYb[pcur];
        float *pxo = last ? nullptr : PXb[pnew], *pyo = last ? nullptr : PYb[pnew];
        float *uo = last ? u_out : free_u(nullptr);
        if (l < nblock) {
            float *upo = last ? nullptr : free_u(uo);
            switch (plan.T) {
            case 2: RC(launch_block<2>(s, u, up, px, py, f, nrows, ncols, frames, plan.c, uo, upo, pxo, pyo)); break;
            case 4: RC(launch_block<4>(s, u, up, px, py, f, nrows, ncols, frames, plan.c, uo, upo, pxo, pyo)); break;
            default: RC(launch_block<8>(s, u, up, px, py, f, nrows, ncols, frames, plan.c, uo, upo, pxo, pyo)); break;
            }
            up = upo;
        } else {
            hipLaunchKernelGGL(k_tvpd_step, pixel_grid(nrows, ncols, frames), dim3(BLOCK), 0, s, u, up, px, py, f, nrows, ncols, plan.c, uo, pxo, pyo);
            up = u;
        }
        u = uo;
        pcur = pnew;
    }
    HIPCHK(hipGetLastError());
    *launches += total;
    return PDEIP_OK;
}

} // namespace

// Launches: see the head of this file.  Workspace (WS_TVPD): eight planes; the start's fill uses WS_EDT.
extern "C" int pdeip_tv_pd_dev(void *stream, const float *f, const float *u0, int nrows, int ncols, int frames, const pdeip_tvpd_params *prm,
                               float *u_out)
{
    const char *who = "pdeip_tv_pd_dev";
    Plan plan;
    RC(tvpd_args(who, f, u0, nrows, ncols, frames, prm, u_out, &plan));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t N = (size_t)nrows * ncols * frames, pN = pad4(N);
    // the workspace: the iteration's eight planes, then the start when it has to be made
    float *ws = nullptr;
    RC(ws_get(WS_TVPD, 9 * pN * sizeof(float), &ws));
    int launches = 0;
    const float *start = u0;
    if (u0 == nullptr) {
        float *filled = plan.iter == 0 ? u_out : ws + 8 * pN;
        RC(pdeip_nearest_fill_dev(stream, f, nrows, ncols, frames, 0, filled, nullptr, nullptr));
        launches += tls.last_launches;
        start = filled;
    } else if (plan.iter == 0) {
        RC(copy_d2d(s, u_out, u0, N));
        launches++;
    }
    if (plan.iter > 0) RC(run_tvpd(s, f, start, nrows, ncols, frames, plan, ws, u_out, &launches));
    tls.last_launches = launches;
    return PDEIP_OK;
}

extern "C" int pdeip_tv_pd(const float *f, const float *u0, int nrows, int ncols, int frames, const pdeip_tvpd_params *prm, float *u_out)
{
    const char *who = "pdeip_tv_pd";
    Plan plan;
    RC(tvpd_args(who, f, u0, nrows, ncols, frames, prm, u_out, &plan));
    RC(use_device());
    const size_t N = (size_t)nrows * ncols * frames, pN = pad4(N);
    float *ar = nullptr; // arena: f, u_out, u0
    RC(ws_get(WS_ARENA, 3 * pN * sizeof(float), &ar));
    float *du0 = u0 ? ar + 2 * pN : nullptr;
    HIPCHK(hipMemcpy(ar, f, N * sizeof(float), hipMemcpyHostToDevice));
    if (u0) HIPCHK(hipMemcpy(du0, u0, N * sizeof(float), hipMemcpyHostToDevice));
    RC(pdeip_tv_pd_dev(nullptr, ar, du0, nrows, ncols, frames, prm, ar + pN));
    HIPCHK(hipMemcpy(u_out, ar + pN, N * sizeof(float), hipMemcpyDeviceToHost));
    return PDEIP_OK;
}
