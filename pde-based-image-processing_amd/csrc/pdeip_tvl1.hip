// pdeip_tvl1.hip -- libpdeip.so: the inner iteration of TV-L1 optical flow (pdeip_tvl1_rc_dev, pdeip_tvl1_iterate_dev).
//
// Kernels: csrc/pdeip_tvl1.hpp; the contract: include/pdeip.h.  The calls have no ordering, so pdeip_set_mode does not apply.  Nothing
// is read back and no launch depends on the data.  The whole driver pdeip_flow_tvl1 is in pdeip_drivers.hip.
//
// Launches, as pdeip_last_launch_count() reports them:
//   pdeip_tvl1_rc_dev        1
//   pdeip_tvl1_iterate_dev   iter = 0: 2 (the copies U -> U_out, V -> V_out);  otherwise L = iter / T blocked launches + iter % T single
//                            steps (T = 1: iter single steps), and with P given and L = 1 one copy more (a single launch cannot write
//                            the planes its neighbours still read)
// PDEIP_TVL1_STEPS: unset or 0 the library's choice (DEFAULT_T), 1 single steps, 2 / 4 that block.
//
// Build (build.py): hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -c, one object per translation unit.
#include "pdeip_ctx.hpp"
#include "pdeip_tvl1.hpp"

#include <cmath>

using namespace pdeip;
using namespace pdeip::tvl1;

namespace {

constexpr int MAX_GRID_YZ = 65535;
constexpr int DEFAULT_T = 2; // measured: the fastest form at 1080p and at 4K; T = 4 wins only at 288x384
constexpr int WS_PLANES = 16; // four of u, four of v, two sets of four duals

struct Plan {
    Consts c;
    int iter, T;
};

int tvl1_dims(const char *who, int nrows, int ncols)
{
    if (nrows < 1 || ncols < 1) return set_err(PDEIP_ERR_ARG, "%s: the plane must be at least 1x1 (got %dx%d)", who, nrows, ncols);
    if ((long long)nrows * ncols > 0x7fffffffLL) return set_err(PDEIP_ERR_ARG, "%s: more than 2^31-1 elements", who);
    return PDEIP_OK;
}

} // namespace

namespace pdeip {

// The parameter refusals of pdeip_tvl1_iterate_dev and pdeip_flow_tvl1, without a HIP call; NaN members have been replaced by their
// defaults.
int tvl1_check_params(const char *who, double lambda, double huber, int iter, double tau, double sigma)
{
    if (!(lambda >= 0.0) || !std::isfinite(lambda)) return set_err(PDEIP_ERR_ARG, "%s: lambda must be finite and >= 0 (got %g)", who, lambda);
    if (!(huber >= 0.0) || !std::isfinite(huber)) return set_err(PDEIP_ERR_ARG, "%s: huber must be finite and >= 0 (got %g)", who, huber);
    if (iter < 0) return set_err(PDEIP_ERR_ARG, "%s: iter must be >= 0 (got %d)", who, iter);
    if (!(tau > 0.0) || !std::isfinite(tau)) return set_err(PDEIP_ERR_ARG, "%s: tau must be positive and finite (got %g)", who, tau);
    if (!(sigma > 0.0) || !std::isfinite(sigma)) return set_err(PDEIP_ERR_ARG, "%s: sigma must be positive and finite (got %g)", who, sigma);
    if (tau * sigma * 8.0 > 1.0) return set_err(PDEIP_ERR_ARG, "%s: tau * sigma * 8 must not exceed 1 (got %g)", who, tau * sigma * 8.0);
    return PDEIP_OK;
}

// The iteration's workspace for planes of up to nrows x ncols, so that a coarse-to-fine run grows it once.
int tvl1_reserve(int nrows, int ncols)
{
    float *ws = nullptr;
    return ws_get(WS_TVL1, (size_t)WS_PLANES * pad4((size_t)nrows * ncols) * sizeof(float), &ws);
}

} // namespace pdeip

namespace {

// Everything refused is refused here, before any HIP call.
int iterate_args(const char *who, const float *rc, const float *gx, const float *gy, const float *U, const float *V, const float *P, int nrows,
                 int ncols, const pdeip_tvl1_params *prm, const float *U_out, const float *V_out, Plan *plan)
{
    NONNULL(who, rc); NONNULL(who, gx); NONNULL(who, gy); NONNULL(who, U); NONNULL(who, V); NONNULL(who, prm); NONNULL(who, U_out); NONNULL(who, V_out);
    RC(tvl1_dims(who, nrows, ncols));
    const size_t N = (size_t)nrows * ncols;
    for (const float *out : {U_out, V_out}) {
        if (out == rc || out == gx || out == gy || out == U || out == V) return set_err(PDEIP_ERR_ARG, "%s: an output is an input", who);
        if (P != nullptr && out + N > P && out < P + 4 * N) return set_err(PDEIP_ERR_ARG, "%s: an output lies within P", who);
    }
    if (U_out == V_out) return set_err(PDEIP_ERR_ARG, "%s: U_out is V_out", who);
    if (P != nullptr && (P == rc || P == gx || P == gy || P == U || P == V)) return set_err(PDEIP_ERR_ARG, "%s: P is an input plane", who);
    const double lambda = std::isnan(prm->lambda) ? 15.0 : prm->lambda, huber = std::isnan(prm->huber) ? 0.0 : prm->huber;
    const double tau = std::isnan(prm->tau) ? 0.25 : prm->tau, sigma = std::isnan(prm->sigma) ? 0.5 : prm->sigma;
    RC(tvl1_check_params(who, lambda, huber, prm->iter, tau, sigma));
    if (ncols > MAX_GRID_YZ) return set_err(PDEIP_ERR_UNSUPPORTED, "%s: more than %d columns (got %d): the launch geometry", who, MAX_GRID_YZ, ncols);
    const int steps = env_int("PDEIP_TVL1_STEPS", 0);
    if (steps != 0 && steps != 1 && steps != 2 && steps != 4)
        return set_err(PDEIP_ERR_ARG, "%s: PDEIP_TVL1_STEPS=%d is not a supported block (0, 1, 2, 4)", who, steps);
    plan->T = steps == 0 ? DEFAULT_T : steps;
    // the constants, each formed once in float32
    const float tau_f = (float)tau, sigma_f = (float)sigma, lambda_f = (float)lambda, huber_f = (float)huber;
    Consts &c = plan->c;
    c.sigma = sigma_f;
    c.tau = tau_f;
    c.tl = tau_f * lambda_f;
    const float sh = sigma_f * huber_f;
    c.hub_den = 1.0f + sh;
    c.huber = huber_f > 0.0f;
    plan->iter = prm->iter;
    return PDEIP_OK;
}

template <int T>
int launch_block(hipStream_t s, const float *U, const float *UP, const float *V, const float *VP, const ConstDuals &P, const float *rc, const float *gx,
                 const float *gy, int nrows, int ncols, const Consts &c, float *Uo, float *Vo, float *UPo, float *VPo, const Duals &Po)
{
    const size_t lds = block_lds_bytes<T>();
    RC(ensure_lds(reinterpret_cast<const void *>(&k_tvl1_block<T>), lds));
    const dim3 grid((unsigned)((nrows + TILE_R - 1) / TILE_R), (unsigned)((ncols + TILE_C - 1) / TILE_C));
    hipLaunchKernelGGL(k_tvl1_block<T>, grid, dim3(BLOCK), lds, s, U, UP, V, VP, P, rc, gx, gy, nrows, ncols, c, Uo, Vo, UPo, VPo, Po);
    return PDEIP_OK;
}

Duals duals_at(float *base, size_t N) { return base ? Duals{base, base + N, base + 2 * N, base + 3 * N} : Duals{nullptr, nullptr, nullptr, nullptr}; }
ConstDuals as_const(const Duals &d) { return ConstDuals{d.pxu, d.pyu, d.pxv, d.pyv}; }

} // namespace

extern "C" int pdeip_tvl1_rc_dev(void *stream, const float *I0, const float *W, const float *gx, const float *gy, const float *U0, const float *V0,
                                 int nrows, int ncols, float *rc)
{
    const char *who = "pdeip_tvl1_rc_dev";
    NONNULL(who, I0); NONNULL(who, W); NONNULL(who, gx); NONNULL(who, gy); NONNULL(who, U0); NONNULL(who, V0); NONNULL(who, rc);
    RC(tvl1_dims(who, nrows, ncols));
    if (rc == I0 || rc == W || rc == gx || rc == gy || rc == U0 || rc == V0) return set_err(PDEIP_ERR_ARG, "%s: rc is an input", who);
    if (ncols > MAX_GRID_YZ) return set_err(PDEIP_ERR_UNSUPPORTED, "%s: more than %d columns (got %d): the launch geometry", who, MAX_GRID_YZ, ncols);
    hipLaunchKernelGGL(k_tvl1_rc, pixel_grid(nrows, ncols, 1), dim3(BLOCK), 0, static_cast<hipStream_t>(stream), I0, W, gx, gy, U0, V0, nrows, ncols, rc);
    HIPCHK(hipGetLastError());
    tls.last_launches = 1;
    return PDEIP_OK;
}

// Launches: see the head of this file.  Workspace (WS_TVL1): sixteen planes.
extern "C" int pdeip_tvl1_iterate_dev(void *stream, const float *rc, const float *gx, const float *gy, const float *U, const float *V, float *P,
                                      int nrows, int ncols, const pdeip_tvl1_params *prm, float *U_out, float *V_out)
{
    const char *who = "pdeip_tvl1_iterate_dev";
    Plan plan;
    RC(iterate_args(who, rc, gx, gy, U, V, P, nrows, ncols, prm, U_out, V_out, &plan));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t N = (size_t)nrows * ncols, pN = pad4(N);
    if (plan.iter == 0) {
        RC(copy_d2d(s, U_out, U, N));
        RC(copy_d2d(s, V_out, V, N));
        tls.last_launches = 2;
        return PDEIP_OK;
    }
    float *ws = nullptr;
    RC(ws_get(WS_TVL1, (size_t)WS_PLANES * pN * sizeof(float), &ws));
    float *Ub[4] = {ws, ws + pN, ws + 2 * pN, ws + 3 * pN}, *Vb[4] = {ws + 4 * pN, ws + 5 * pN, ws + 6 * pN, ws + 7 * pN};
    float *sets[2] = {ws + 8 * pN, ws + 12 * pN}; // four planes of N each, contiguous like P
    const float *u = U, *up = U, *v = V, *vp = V;
    ConstDuals pin = as_const(duals_at(P, N));
    const int nblock = plan.T > 1 ? plan.iter / plan.T : 0, nstep = plan.iter - nblock * plan.T, total = nblock + nstep;
    const bool copy_back = P != nullptr && total == 1; // a single launch reads P's neighbours: it cannot write P
    const auto free_buf = [&](int not_this) { // a buffer that holds neither the iterate nor its predecessor
        int k = 0;
        while (Ub[k] == u || Ub[k] == up || k == not_this) k++;
        return k;
    };
    for (int l = 0; l < total; l++) {
        const bool last = l == total - 1;
        const int ko = free_buf(-1);
        float *uo = last ? U_out : Ub[ko], *vo = last ? V_out : Vb[ko];
        float *pout = !last || copy_back ? sets[l & 1] : P; // the last launch: P, or NULL when the duals are not handed on
        const Duals po = duals_at(pout, N);
        if (l < nblock) {
            const int kp = last ? -1 : free_buf(ko);
            float *upo = last ? nullptr : Ub[kp], *vpo = last ? nullptr : Vb[kp];
            if (plan.T == 2) RC(launch_block<2>(s, u, up, v, vp, pin, rc, gx, gy, nrows, ncols, plan.c, uo, vo, upo, vpo, po));
            else RC(launch_block<4>(s, u, up, v, vp, pin, rc, gx, gy, nrows, ncols, plan.c, uo, vo, upo, vpo, po));
            up = upo;
            vp = vpo;
        } else {
            hipLaunchKernelGGL(k_tvl1_step, pixel_grid(nrows, ncols, 1), dim3(BLOCK), 0, s, u, up, v, vp, pin, rc, gx, gy, nrows, ncols, plan.c, uo, vo, po);
            up = u;
            vp = v;
        }
        u = uo;
        v = vo;
        pin = as_const(po);
    }
    HIPCHK(hipGetLastError());
    if (copy_back) RC(copy_d2d(s, P, sets[0], 4 * N));
    tls.last_launches = total + (copy_back ? 1 : 0);
    return PDEIP_OK;
}
