// pdeip_levelset.hip -- libpdeip.so: the level-set gateways of the active-contour section of runme.m.
//
//   PHI_out = AC_solver_2d(PHI, D, GradNorm, Diff, tau, nu)   mex/source/AC_solver_2d.c -> AC_AOS_4_2d   pdeip_ac_solver(_dev)
//   PHI_out = Reinit(PHI, T)                                  mex/source/Reinit.c       -> reinit         pdeip_reinit(_dev)
//   PHI_out = CV_solver_2d(PHI, D, DH, GradNorm, tau, nu)     mex/source/CV_solver_2d.c -> CV_AOSOMP_4_2d pdeip_cv_solver(_dev)
//   [DH, gradPHI] of the segmentation drivers                                                            pdeip_cv_terms(_dev)
//   PHIout = GAC_v10a / GAC_v10b(Iin, PHIin, ...)             matlab/active_contour/GAC_v10{a,b}.m      pdeip_gac(_dev)
//   sort(x)(k) and [Igrad, lambda, g] of those drivers: the stages before their loop                     pdeip_select_kth_dev, pdeip_gac_stopping_dev
//
// Kernels: csrc/pdeip_levelset.hpp, csrc/pdeip_cv.hpp; their line solve and its grid: csrc/pdeip_thomas.hpp.  AOS has one order,
// so pdeip_set_mode does not apply.  Multi-frame inputs are planes solved independently, as in the reference.  Lines of any length
// are accepted (the reference stops at MAX_BUF_SIZE = 2048).
//
// Build (build.py): hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -c, one object per translation unit.
#include "pdeip_ctx.hpp"
#include "pdeip_levelset.hpp"
#include "pdeip_cv.hpp"

#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

using namespace pdeip;
using namespace pdeip::ls;

namespace {

// nrows, ncols >= 2: at 1 the reference reads outside the line (undefined behaviour), so it is refused before any HIP call.
int check_ls_dims(const char *who, int nrows, int ncols, int nframes)
{
    if (nrows < 2 || ncols < 2)
        return set_err(PDEIP_ERR_ARG, "%s: PHI must be at least 2x2 (got %dx%d)", who, nrows, ncols);
    if (nframes < 1) return set_err(PDEIP_ERR_ARG, "%s: number of frames must be >= 1 (got %d)", who, nframes);
    if ((long long)nrows * ncols * nframes > 0x7fffffffLL) return set_err(PDEIP_ERR_ARG, "%s: more than 2^31-1 elements", who);
    return PDEIP_OK;
}

// Steps of the reference's loop `for (t = 0.0f; t < T; t += 0.25f)` (levelsetSolvers.c:1076): T <= 0 or NaN gives none.
// Where t + 0.25f no longer changes t the reference never ends; that T is refused.
int reinit_step_count(const char *who, float T, int *steps)
{
    int n = 0;
    for (float t = 0.0f; t < T; t += 0.25f) {
        if (t + 0.25f == t || n == 0x7fffffff) return set_err(PDEIP_ERR_ARG, "%s: T = %g never ends the reference's time loop", who, (double)T);
        n++;
    }
    *steps = n;
    return PDEIP_OK;
}

int launch_reinit_step(hipStream_t s, const float *in, float *out, int nrows, int ncols, int nframes)
{
    hipLaunchKernelGGL(k_reinit_step, pixel_grid(nrows, ncols, nframes), dim3(256), 0, s, in, out, nrows, ncols);
    HIPCHK(hipGetLastError());
    tls.last_launches++;
    return PDEIP_OK;
}

int upload(float *dst, const float *src, size_t n)
{
    HIPCHK(hipMemcpy(dst, src, n * sizeof(float), hipMemcpyHostToDevice));
    return PDEIP_OK;
}

} // namespace

extern "C" int pdeip_ac_solver_dev(void *stream, const float *PHI, const float *D, const float *GradNorm, const float *Diff,
                                   int nrows, int ncols, int nframes, float tau, float nu, float *PHI_out)
{
    const char *who = "pdeip_ac_solver_dev";
    NONNULL(who, PHI); NONNULL(who, D); NONNULL(who, GradNorm); NONNULL(who, Diff); NONNULL(who, PHI_out);
    RC(check_ls_dims(who, nrows, ncols, nframes));
    if (PHI_out == PHI || PHI_out == D || PHI_out == GradNorm || PHI_out == Diff)
        return set_err(PDEIP_ERR_ARG, "%s: PHI_out must not alias an input", who);
    tls.last_launches = 0;
    const size_t nf = (size_t)nrows * ncols * nframes;
    float *ws = nullptr;
    RC(ws_get(WS_LS, pad4(nf) * 3 * sizeof(float), &ws));
    float *cp = ws, *dp = ws + pad4(nf), *sum = ws + 2 * pad4(nf);
    hipStream_t s = static_cast<hipStream_t>(stream);
    // column pass -> PHI_out (AC_TDMA_column4), row pass -> sum (AC_TDMA_row4), one re-initialisation step -> PHI_out (:178)
    hipLaunchKernelGGL(k_aos_col, dim3((unsigned)thomas::line_blocks(ncols), (unsigned)nframes), dim3(thomas::BLOCK), 0, s,
                       PHI, D, GradNorm, Diff, PHI_out, cp, dp, nrows, ncols, tau, nu);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_aos_row, dim3((unsigned)thomas::line_blocks(nrows), (unsigned)nframes), dim3(thomas::BLOCK), 0, s,
                       PHI, D, GradNorm, Diff, PHI_out, sum, cp, dp, nrows, ncols, tau, nu);
    HIPCHK(hipGetLastError());
    tls.last_launches += 2;
    return launch_reinit_step(s, sum, PHI_out, nrows, ncols, nframes);
}

extern "C" int pdeip_reinit_dev(void *stream, const float *PHI, int nrows, int ncols, int nframes, float T, float *PHI_out)
{
    const char *who = "pdeip_reinit_dev";
    NONNULL(who, PHI); NONNULL(who, PHI_out);
    RC(check_ls_dims(who, nrows, ncols, nframes));
    if (PHI_out == PHI) return set_err(PDEIP_ERR_ARG, "%s: PHI_out must not alias PHI", who);
    int steps = 0;
    RC(reinit_step_count(who, T, &steps));
    tls.last_launches = 0;
    const size_t nf = (size_t)nrows * ncols * nframes;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (steps == 0) return copy_d2d(s, PHI_out, PHI, nf);
    float *scr = nullptr;
    if (steps > 1) RC(ws_get(WS_LS, pad4(nf) * sizeof(float), &scr));
    // ping-pong so that the last step lands in PHI_out; PHI itself is never written
    const float *src = PHI;
    for (int k = 0; k < steps; k++) {
        float *dst = ((steps - k) & 1) ? PHI_out : scr;
        RC(launch_reinit_step(s, src, dst, nrows, ncols, nframes));
        src = dst;
    }
    return PDEIP_OK;
}

extern "C" int pdeip_ac_solver(const float *PHI, const float *D, const float *GradNorm, const float *Diff, int nrows, int ncols,
                               int nframes, float tau, float nu, float *PHI_out)
{
    const char *who = "AC_solver_2D";
    NONNULL(who, PHI); NONNULL(who, D); NONNULL(who, GradNorm); NONNULL(who, Diff); NONNULL(who, PHI_out);
    RC(check_ls_dims(who, nrows, ncols, nframes));
    RC(use_device());
    const size_t nf = (size_t)nrows * ncols * nframes, p = pad4(nf);
    float *ar = nullptr;
    RC(ws_get(WS_ARENA, p * 5 * sizeof(float), &ar));
    float *dP = ar, *dD = ar + p, *dG = ar + 2 * p, *dF = ar + 3 * p, *dO = ar + 4 * p;
    RC(upload(dP, PHI, nf)); RC(upload(dD, D, nf)); RC(upload(dG, GradNorm, nf)); RC(upload(dF, Diff, nf));
    RC(pdeip_ac_solver_dev(nullptr, dP, dD, dG, dF, nrows, ncols, nframes, tau, nu, dO));
    HIPCHK(hipMemcpy(PHI_out, dO, nf * sizeof(float), hipMemcpyDeviceToHost));
    return PDEIP_OK;
}

// Unlike Reinit.c:136-137, which re-initialises its input array in place before copying it out, PHI is left as it was.
extern "C" int pdeip_reinit(const float *PHI, int nrows, int ncols, int nframes, float T, float *PHI_out)
{
    const char *who = "reInitC";
    NONNULL(who, PHI); NONNULL(who, PHI_out);
    RC(check_ls_dims(who, nrows, ncols, nframes));
    int steps = 0;
    RC(reinit_step_count(who, T, &steps));
    const size_t nf = (size_t)nrows * ncols * nframes, p = pad4(nf);
    if (steps == 0) { // nothing to compute: the output is the input
        if (PHI_out != PHI) memcpy(PHI_out, PHI, nf * sizeof(float));
        return PDEIP_OK;
    }
    RC(use_device());
    float *ar = nullptr;
    RC(ws_get(WS_ARENA, p * 2 * sizeof(float), &ar));
    float *dP = ar, *dO = ar + p;
    RC(upload(dP, PHI, nf));
    RC(pdeip_reinit_dev(nullptr, dP, nrows, ncols, nframes, T, dO));
    HIPCHK(hipMemcpy(PHI_out, dO, nf * sizeof(float), hipMemcpyDeviceToHost));
    return PDEIP_OK;
}

// ---- PHIout = GAC_v10a(Iin, PHIin, ...) / GAC_v10b(...): the whole driver, resident ------------------------------------------
// matlab/active_contour/GAC_v10a.m:35-121 and GAC_v10b.m.  Reinit(PHIin, 10); imfilter(Iin, fspecial('gaussian',[7 7],2.5),
// 'replicate') per channel and the [-1 0 1]*0.5 derivatives as pyramid.py defines those IPT calls; the largest derivative over
// the channels; lambda = sort(Igrad(:))(round(0.7*N)) selected on the device when param.lambda < 0; g; then `while iter < ITER`
// the model's data term and one AC_solver_2d step.  Nothing is read back to the host inside the run.
namespace {

struct GacPrm {
    double tau, c, lambda, iter, smooth;
};
GacPrm gac_resolve(const pdeip_gac_params *u)
{
    GacPrm p{0.25, -0.1, -1.0, 100.0, 100.0}; // GAC_v10a.m:35-42
    if (u) {
        if (!std::isnan(u->tau)) p.tau = u->tau;
        if (!std::isnan(u->c)) p.c = u->c;
        if (!std::isnan(u->lambda)) p.lambda = u->lambda;
        if (!std::isnan(u->iter)) p.iter = u->iter;
        if (!std::isnan(u->smooth)) p.smooth = u->smooth;
    }
    return p;
}

} // namespace

// The k-th smallest (1-based) of x[0..n), NaN last: k_sel_init, then per 8-bit digit of the order-preserving key (most significant first)
// one k_sel_hist over x and one k_sel_pick.  Nine launches; the state lives in its own workspace slot and every call clears it first.
extern "C" int pdeip_select_kth_dev(void *stream, const float *x, long long n, long long k, float *out)
{
    const char *who = "pdeip_select_kth_dev";
    NONNULL(who, x); NONNULL(who, out);
    if (n < 1 || n > 0x7fffffffLL) return set_err(PDEIP_ERR_ARG, "%s: n must be in 1 .. 2^31-1 (got %lld)", who, n);
    if (k < 1 || k > n) return set_err(PDEIP_ERR_ARG, "%s: k must be in 1 .. n (got %lld of %lld)", who, k, n);
    float *ws = nullptr;
    RC(ws_get(WS_SELECT, sizeof(Select), &ws));
    Select *sel = reinterpret_cast<Select *>(ws);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_sel_init, dim3(1), dim3(256), 0, s, sel, (unsigned)k);
    const unsigned blocks = (unsigned)std::min<size_t>(((size_t)n + 255) / 256, 1024);
    for (int shift = 24; shift >= 0; shift -= 8) {
        hipLaunchKernelGGL(k_sel_hist, dim3(blocks), dim3(256), 0, s, sel, x, (size_t)n, shift);
        hipLaunchKernelGGL(k_sel_pick, dim3(1), dim3(64), 0, s, sel, shift, out);
    }
    HIPCHK(hipGetLastError());
    tls.last_launches = 9;
    return PDEIP_OK;
}

namespace {
int check_gac_dims(const char *who, int nrows, int ncols, int channels)
{
    if (nrows < 3 || ncols < 3) return set_err(PDEIP_ERR_ARG, "%s: image must be at least 3x3 (got %dx%d)", who, nrows, ncols);
    if (channels < 1) return set_err(PDEIP_ERR_ARG, "%s: number of channels must be >= 1 (got %d)", who, channels);
    if ((long long)nrows * ncols * (channels + 9) > 0x7fffffffLL) return set_err(PDEIP_ERR_ARG, "%s: image too large", who);
    return PDEIP_OK;
}
} // namespace

// Igrad, lambda and g of the drivers (GAC_v10a.m:57-75): the smoothing, k_gac_igrad, the selection when lambda < 0, k_gac_g.
extern "C" int pdeip_gac_stopping_dev(void *stream, const float *I, int nrows, int ncols, int channels, double lambda, float *Igrad_out,
                                      float *g_out, float *lambda_out)
{
    const char *who = "pdeip_gac_stopping_dev";
    NONNULL(who, I); NONNULL(who, Igrad_out); NONNULL(who, g_out); NONNULL(who, lambda_out);
    RC(check_gac_dims(who, nrows, ncols, channels));
    if (Igrad_out == I || g_out == I || Igrad_out == g_out) return set_err(PDEIP_ERR_ARG, "%s: Igrad_out and g_out must not alias I or each other", who);
    const size_t n = (size_t)nrows * ncols, pn = pad4(n);
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *Ism = nullptr;
    RC(ws_get(WS_GAC, pn * (size_t)channels * sizeof(float), &Ism));
    const std::vector<double> G = gaussian_mask(7, 2.5);
    RC(pdeip_pyr_smooth_dev(s, I, nrows, ncols, channels, G.data(), 7, Ism));
    hipLaunchKernelGGL(k_gac_igrad, pixel_grid(nrows, ncols, 1), dim3(256), 0, s, Ism, Igrad_out, nrows, ncols, channels);
    HIPCHK(hipGetLastError());
    int launches = 2;
    const float *lam_dev = nullptr;
    if (lambda < 0.0) {
        const double kd = std::round(0.7 * (double)n); // MATLAB round: half away from zero; 1-based rank
        RC(pdeip_select_kth_dev(s, Igrad_out, (long long)n, kd < 1.0 ? 1LL : (long long)kd, lambda_out));
        launches += tls.last_launches;
        lam_dev = lambda_out;
    }
    hipLaunchKernelGGL(k_gac_g, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, Igrad_out, g_out, n, lam_dev, (float)lambda, lambda_out);
    HIPCHK(hipGetLastError());
    tls.last_launches = launches + 1;
    return PDEIP_OK;
}

extern "C" int pdeip_gac_dev(void *stream, const float *Iin, int nrows, int ncols, int channels, const float *PHIin, int model,
                             const pdeip_gac_params *prm, float *PHIout)
{
    const char *who = "pdeip_gac_dev";
    NONNULL(who, Iin); NONNULL(who, PHIin); NONNULL(who, PHIout);
    RC(check_gac_dims(who, nrows, ncols, channels));
    if (model != PDEIP_GAC_A && model != PDEIP_GAC_B) return set_err(PDEIP_ERR_ARG, "%s: model must be PDEIP_GAC_A or PDEIP_GAC_B", who);
    const GacPrm p = gac_resolve(prm);
    if (!(p.iter < 2147483647.0)) return set_err(PDEIP_ERR_ARG, "%s: ITER = %g is too large", who, p.iter);
    const int iters = p.iter > 0.0 ? (int)std::ceil(p.iter) : 0; // iterations of `iter = 0; while iter < ITER`
    const size_t n = (size_t)nrows * ncols, pn = pad4(n);
    hipStream_t s = static_cast<hipStream_t>(stream);

    float *ws = nullptr;
    RC(ws_get(WS_DRIVER, (pn * 9 + 4) * sizeof(float), &ws)); // the smoothed channels and the selection state: pdeip_gac_stopping_dev's
    float *Igrad = ws, *g = Igrad + pn, *gdx = g + pn, *gdy = gdx + pn, *P0 = gdy + pn, *P1 = P0 + pn;
    float *DATA = P1 + pn, *gradPHI = DATA + pn, *Diff = gradPHI + pn, *lam = Diff + pn;
    int launches = 0;

    RC(pdeip_reinit_dev(s, PHIin, nrows, ncols, 1, 10.0f, P0)); // Reinit(single(PHIin), single(10)): 40 steps
    launches += tls.last_launches;
    RC(pdeip_gac_stopping_dev(s, Iin, nrows, ncols, channels, p.lambda, Igrad, g, lam));
    launches += tls.last_launches;
    const dim3 grid = pixel_grid(nrows, ncols, 1), blk(256);
    if (model == PDEIP_GAC_B) {
        hipLaunchKernelGGL(k_gac_gd, grid, blk, 0, s, g, gdx, gdy, nrows, ncols);
        launches++;
    }
    HIPCHK(hipGetLastError());
    float *cur = P0, *nxt = P1;
    for (int it = 0; it < iters; it++) {
        if (model == PDEIP_GAC_A)
            hipLaunchKernelGGL(k_gac_terms<0>, grid, blk, 0, s, cur, g, gdx, gdy, (float)p.c, p.c <= 0.0 ? 1 : 0, DATA, gradPHI, Diff, nrows, ncols);
        else
            hipLaunchKernelGGL(k_gac_terms<1>, grid, blk, 0, s, cur, g, gdx, gdy, (float)p.c, 0, DATA, gradPHI, Diff, nrows, ncols);
        HIPCHK(hipGetLastError());
        RC(pdeip_ac_solver_dev(s, cur, DATA, gradPHI, Diff, nrows, ncols, 1, (float)p.tau, (float)p.smooth, nxt));
        launches += 1 + tls.last_launches;
        std::swap(cur, nxt);
    }
    RC(copy_d2d(s, PHIout, cur, n));
    tls.last_launches = launches + 1;
    return PDEIP_OK;
}

extern "C" int pdeip_gac(const float *Iin, int nrows, int ncols, int channels, const float *PHIin, int model,
                         const pdeip_gac_params *prm, float *PHIout)
{
    const char *who = "pdeip_gac";
    NONNULL(who, Iin); NONNULL(who, PHIin); NONNULL(who, PHIout);
    if (nrows < 3 || ncols < 3) return set_err(PDEIP_ERR_ARG, "%s: image must be at least 3x3 (got %dx%d)", who, nrows, ncols);
    if (channels < 1) return set_err(PDEIP_ERR_ARG, "%s: number of channels must be >= 1 (got %d)", who, channels);
    if (model != PDEIP_GAC_A && model != PDEIP_GAC_B) return set_err(PDEIP_ERR_ARG, "%s: model must be PDEIP_GAC_A or PDEIP_GAC_B", who);
    RC(use_device());
    const size_t n = (size_t)nrows * ncols, p = pad4(n);
    float *ar = nullptr;
    RC(ws_get(WS_ARENA, p * ((size_t)channels + 2) * sizeof(float), &ar));
    float *dI = ar, *dP = ar + p * channels, *dO = dP + p;
    RC(upload(dI, Iin, n * channels));
    RC(upload(dP, PHIin, n));
    RC(pdeip_gac_dev(nullptr, dI, nrows, ncols, channels, dP, model, prm, dO));
    HIPCHK(hipMemcpy(PHIout, dO, n * sizeof(float), hipMemcpyDeviceToHost));
    return PDEIP_OK;
}

// ---- PHI_out = CV_solver_2d(PHI, D, DH, GradNorm, tau, nu): the Chan-Vese AOS step (csrc/pdeip_cv.hpp) --------------------------
extern "C" int pdeip_cv_solver_dev(void *stream, const float *PHI, const float *D, const float *DH, const float *GradNorm,
                                   int nrows, int ncols, int nframes, float tau, float nu, float *PHI_out)
{
    const char *who = "pdeip_cv_solver_dev";
    NONNULL(who, PHI); NONNULL(who, D); NONNULL(who, DH); NONNULL(who, GradNorm); NONNULL(who, PHI_out);
    RC(check_ls_dims(who, nrows, ncols, nframes));
    if (PHI_out == PHI || PHI_out == D || PHI_out == DH || PHI_out == GradNorm)
        return set_err(PDEIP_ERR_ARG, "%s: PHI_out must not alias an input", who);
    tls.last_launches = 0;
    const size_t p = pad4((size_t)nrows * ncols * nframes);
    float *ws = nullptr;
    RC(ws_get(WS_LS, p * 6 * sizeof(float), &ws));
    const thomas::Planes w = thomas::carve_planes(ws, p);
    hipStream_t s = static_cast<hipStream_t>(stream);
    // column lanes and row lanes in one grid (their chains do not depend on each other), then the output rules
    hipLaunchKernelGGL(k_cv_lines, thomas::lines_grid(nrows, ncols, nframes), dim3(thomas::BLOCK), 0, s, PHI, D, DH, GradNorm, w.xc,
                       w.xr, w.cpc, w.dpc, w.cpr, w.dpr, nrows, ncols, thomas::line_blocks(nrows), tau, nu);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_cv_combine, pixel_grid(nrows, ncols, nframes), dim3(256), 0, s, PHI, GradNorm, w.xc, w.xr, PHI_out, nrows,
                       ncols);
    HIPCHK(hipGetLastError());
    tls.last_launches = 2;
    return PDEIP_OK;
}

extern "C" int pdeip_cv_solver(const float *PHI, const float *D, const float *DH, const float *GradNorm, int nrows, int ncols,
                               int nframes, float tau, float nu, float *PHI_out)
{
    const char *who = "cv_solver_2D";
    NONNULL(who, PHI); NONNULL(who, D); NONNULL(who, DH); NONNULL(who, GradNorm); NONNULL(who, PHI_out);
    RC(check_ls_dims(who, nrows, ncols, nframes));
    RC(use_device());
    const size_t nf = (size_t)nrows * ncols * nframes, p = pad4(nf);
    float *ar = nullptr;
    RC(ws_get(WS_ARENA, p * 5 * sizeof(float), &ar));
    float *dP = ar, *dD = ar + p, *dH = ar + 2 * p, *dG = ar + 3 * p, *dO = ar + 4 * p;
    RC(upload(dP, PHI, nf)); RC(upload(dD, D, nf)); RC(upload(dH, DH, nf)); RC(upload(dG, GradNorm, nf));
    RC(pdeip_cv_solver_dev(nullptr, dP, dD, dH, dG, nrows, ncols, nframes, tau, nu, dO));
    HIPCHK(hipMemcpy(PHI_out, dO, nf * sizeof(float), hipMemcpyDeviceToHost));
    return PDEIP_OK;
}

namespace {
int check_terms_args(const char *who, const float *PHI, int nrows, int ncols, int nframes, const float *DH_out, const float *G_out)
{
    if (nrows < 1 || ncols < 1 || nframes < 1)
        return set_err(PDEIP_ERR_ARG, "%s: PHI must not be empty (got %dx%dx%d)", who, nrows, ncols, nframes);
    if ((long long)nrows * ncols * nframes > 0x7fffffffLL) return set_err(PDEIP_ERR_ARG, "%s: more than 2^31-1 elements", who);
    if (DH_out == PHI || G_out == PHI || DH_out == G_out)
        return set_err(PDEIP_ERR_ARG, "%s: DH_out and GradNorm_out must not alias PHI or each other", who);
    return PDEIP_OK;
}
} // namespace

extern "C" int pdeip_cv_terms_dev(void *stream, const float *PHI, int nrows, int ncols, int nframes, float c0, float c1, float dh_floor,
                                  float *DH_out, float *GradNorm_out)
{
    const char *who = "pdeip_cv_terms_dev";
    NONNULL(who, PHI); NONNULL(who, DH_out); NONNULL(who, GradNorm_out);
    RC(check_terms_args(who, PHI, nrows, ncols, nframes, DH_out, GradNorm_out));
    hipLaunchKernelGGL(k_cv_terms, pixel_grid(nrows, ncols, nframes), dim3(256), 0, static_cast<hipStream_t>(stream), PHI, DH_out,
                       GradNorm_out, nrows, ncols, c0, c1, dh_floor);
    HIPCHK(hipGetLastError());
    tls.last_launches = 1;
    return PDEIP_OK;
}

extern "C" int pdeip_cv_terms(const float *PHI, int nrows, int ncols, int nframes, float c0, float c1, float dh_floor, float *DH_out,
                              float *GradNorm_out)
{
    const char *who = "pdeip_cv_terms";
    NONNULL(who, PHI); NONNULL(who, DH_out); NONNULL(who, GradNorm_out);
    RC(check_terms_args(who, PHI, nrows, ncols, nframes, DH_out, GradNorm_out));
    RC(use_device());
    const size_t nf = (size_t)nrows * ncols * nframes, p = pad4(nf);
    float *ar = nullptr;
    RC(ws_get(WS_ARENA, p * 3 * sizeof(float), &ar));
    float *dP = ar, *dH = ar + p, *dG = ar + 2 * p;
    RC(upload(dP, PHI, nf));
    RC(pdeip_cv_terms_dev(nullptr, dP, nrows, ncols, nframes, c0, c1, dh_floor, dH, dG));
    HIPCHK(hipMemcpy(DH_out, dH, nf * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(GradNorm_out, dG, nf * sizeof(float), hipMemcpyDeviceToHost));
    return PDEIP_OK;
}
