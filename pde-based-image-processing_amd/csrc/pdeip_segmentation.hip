// pdeip_segmentation.hip -- libpdeip.so: region competition, the inner loop of the segmentation drivers.
//
//   regionCompetition() between its MEX calls   matlab/segmentation/DispSegmentation.m:497-646, DispSegmentationSparse.m:511-666
//     sizes, variance, likelihood + competitor + data term                pdeip_seg_sizes_dev / _variance_dev / _data_dev
//     `iterations` competition iterations on one scale, resident          pdeip_seg_competition_level(_dev)
//     the whole regionCompetition() over its scale pyramid                pdeip_region_competition
//   the numbered segment map (DispSegmentation.m:190-198)                 pdeip_seg_label(_dev)
//   generateSeeds() (DispSegmentation.m:203-443)                          pdeip_generate_seeds
//   the dense driver (DispSegmentation.m:31-198)                          pdeip_disp_segmentation
//   the sparse driver (DispSegmentationSparse.m:42-202) and its two stages    pdeip_disp_segmentation_sparse, pdeip_generate_seeds_sparse,
//                                                                         pdeip_region_competition_sparse
// Each dense / sparse pair shares one body: which builder makes the D pyramid, the constants a NaN member or a NULL struct resolves to
// and generateSeeds()'s starting gamma are passed in (Form below).
//
// Kernels: csrc/pdeip_segmentation.hpp; the seed loop's host-side schedule: csrc/pdeip_seeds_plan.hpp, the sparse forms' plan:
// csrc/pdeip_sparse_plan.hpp (the pyramid itself: csrc/pdeip_sparse.hip); the contract: include/pdeip.h.  The fit is
// pdeip_surface_fit_masked_batch_dev (a level: all live segments in one chain) or pdeip_surface_fit_masked_dev (generateSeeds: one
// segment at a time), the terms and the step pdeip_cv_terms_dev / pdeip_cv_solver_dev.  pdeip_set_mode does not apply.
//
// Build (build.py): hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -c, one object per translation unit.
#include "pdeip_ctx.hpp"
#include "pdeip_segmentation.hpp"
#include "pdeip_seeds_plan.hpp"
#include "pdeip_sparse_plan.hpp"

#include <algorithm>
#include <cmath>
#include <limits>
#include <utility>
#include <vector>

using namespace pdeip;
using namespace pdeip::seg;

namespace {

struct SegPrm {
    float c0, c1, dh_floor, err_thr;
    double gamma_coef, dist_cap;
    float nan_fill;
};
SegPrm seg_resolve(const pdeip_seg_params *u, bool sparse = false)
{
    SegPrm p{1.0f, 1.0f, 0.06f, 1.0f, 0.001, std::numeric_limits<double>::infinity(), std::numeric_limits<float>::quiet_NaN()}; // DispSegmentation.m
    if (sparse) p = SegPrm{2.0f, 4.0f, 0.04f, 1.2f, 0.005, 100.0, 1000.0f}; // DispSegmentationSparse.m
    if (u) {
        if (!std::isnan(u->c0)) p.c0 = (float)u->c0;
        if (!std::isnan(u->c1)) p.c1 = (float)u->c1;
        if (!std::isnan(u->dh_floor)) p.dh_floor = (float)u->dh_floor;
        if (!std::isnan(u->err_thr)) p.err_thr = (float)u->err_thr;
        if (!std::isnan(u->gamma_coef)) p.gamma_coef = u->gamma_coef;
        if (!std::isnan(u->dist_cap)) p.dist_cap = u->dist_cap;
        if (!std::isnan(u->nan_fill)) p.nan_fill = (float)u->nan_fill;
    }
    return p;
}

int check_planes(const char *who, int nrows, int ncols, int S)
{
    if (nrows < 2 || ncols < 2) return set_err(PDEIP_ERR_ARG, "%s: planes must be at least 2x2 (got %dx%d)", who, nrows, ncols);
    if (S < 1 || S > 65535) return set_err(PDEIP_ERR_ARG, "%s: number of segments must lie in 1..65535 (got %d)", who, S);
    if ((long long)nrows * ncols > 0x7fffffffLL / 8 || (long long)nrows * ncols * S > 0x7fffffffLL / 8)
        return set_err(PDEIP_ERR_ARG, "%s: planes too large", who);
    return PDEIP_OK;
}

int check_strategy(const char *who, int strategy)
{
    if (strategy != PDEIP_SEG_SURFACE && strategy != PDEIP_SEG_GREEDY && strategy != PDEIP_SEG_INVERSE)
        return set_err(PDEIP_ERR_ARG, "%s: no such competition strategy (%d)", who, strategy);
    return PDEIP_OK;
}

int check_level(const char *who, int nrows, int ncols, int S, int order, int strategy, double minCOV, float ransac_cset, int iterations,
                double srem_thr, const SegPrm &p)
{
    RC(check_planes(who, nrows, ncols, S));
    if (order != 1 && order != 2) return set_err(PDEIP_ERR_ARG, "%s: only 1st and 2nd order polynomials are implemented (order = %d)", who, order);
    RC(check_strategy(who, strategy));
    if (!std::isfinite(minCOV) || !std::isfinite(srem_thr) || !std::isfinite(p.err_thr) || !std::isfinite(ransac_cset))
        return set_err(PDEIP_ERR_ARG, "%s: minCOV, srem_thr, err_thr and ransac_cset must be finite", who);
    if (minCOV <= 0.0) return set_err(PDEIP_ERR_ARG, "%s: minCOV must be > 0 (got %g)", who, minCOV);
    if (iterations < 0) return set_err(PDEIP_ERR_ARG, "%s: iterations must be >= 0 (got %d)", who, iterations);
    return PDEIP_OK;
}

inline int tiles_of(int npix) { return (npix + SG_BLOCK - 1) / SG_BLOCK; }

int launch_sizes(hipStream_t s, const float *PHI, int npix, int S, int *part, int *sizes)
{
    const int tiles = tiles_of(npix);
    hipLaunchKernelGGL(k_seg_sizes, dim3((unsigned)tiles, (unsigned)S), dim3(SG_BLOCK), 0, s, PHI, npix, tiles, part);
    hipLaunchKernelGGL(k_seg_sizes_final, dim3((unsigned)S), dim3(SG_FIN_BLOCK), 0, s, part, tiles, sizes);
    HIPCHK(hipGetLastError());
    return PDEIP_OK;
}

int launch_variance(hipStream_t s, const float *PHI, const float *dist, int npix, int S, double minCOV, double dist_cap, double *psum, int *pcnt,
                    double *cov, int *n_out)
{
    const int tiles = tiles_of(npix);
    hipLaunchKernelGGL(k_seg_variance, dim3((unsigned)tiles, (unsigned)S), dim3(SG_BLOCK), 0, s, PHI, dist, npix, tiles, std::isfinite(dist_cap) ? 1 : 0,
                       dist_cap, psum, pcnt);
    hipLaunchKernelGGL(k_seg_variance_final, dim3(1), dim3(SG_FIN_BLOCK), 0, s, psum, pcnt, tiles, S, minCOV, cov, n_out);
    HIPCHK(hipGetLastError());
    return PDEIP_OK;
}

int launch_data(hipStream_t s, const float *dist, const float *PHI, const float *DH, const double *cov, int npix, int S, int strategy, float *DATA,
                double *P_out)
{
    const dim3 grid((unsigned)tiles_of(npix)), blk(SG_BLOCK);
    if (strategy == PDEIP_SEG_SURFACE) hipLaunchKernelGGL(k_seg_data<STRAT_SURFACE>, grid, blk, 0, s, dist, PHI, DH, cov, npix, S, DATA, P_out);
    else if (strategy == PDEIP_SEG_GREEDY) hipLaunchKernelGGL(k_seg_data<STRAT_GREEDY>, grid, blk, 0, s, dist, PHI, DH, cov, npix, S, DATA, P_out);
    else hipLaunchKernelGGL(k_seg_data<STRAT_INVERSE>, grid, blk, 0, s, dist, PHI, DH, cov, npix, S, DATA, P_out);
    HIPCHK(hipGetLastError());
    return PDEIP_OK;
}

// Partials of the stage calls: [S * tiles] doubles, then as many ints.
int stage_ws(int npix, int S, double **psum, int **pcnt)
{
    const size_t np = (size_t)S * tiles_of(npix);
    float *ws = nullptr;
    RC(ws_get(WS_SEG_STAGE, (2 * np + pad4(np)) * sizeof(float), &ws));
    *psum = reinterpret_cast<double *>(ws);
    *pcnt = reinterpret_cast<int *>(ws + 2 * np);
    return PDEIP_OK;
}

// The pinned words the level reads the sizes back through, grown on demand and kept for the life of the process.
int *g_pinned = nullptr;
int g_pinned_cap = 0;
int pinned_sizes(int S, int **out)
{
    if (S > g_pinned_cap) {
        if (g_pinned) HIPCHK(hipHostFree(g_pinned));
        g_pinned = nullptr;
        g_pinned_cap = 0;
        HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&g_pinned), (size_t)std::max(S, 64) * sizeof(int), hipHostMallocDefault));
        g_pinned_cap = std::max(S, 64);
    }
    *out = g_pinned;
    return PDEIP_OK;
}

// What the two drivers' stages differ in beyond their parameter structs.
struct Form {
    bool sparse;   // the D pyramid: plain cubic resizes of D, or nanmedfilt2 around every step (sparse_pyramid_dev)
    double gamma0; // generateSeeds()'s starting gamma
};
constexpr Form DENSE_FORM{false, seeds::GAMMA0}, SPARSE_FORM{true, sparse::GAMMA0};

// Floats the D pyramid's builder needs beside the K planes: none for the plain form, a staging plane for the raw D and the two
// temporaries for the sparse one.
template <class Sizes>
size_t pyramid_extra(const Form &f, const Sizes &sz, int K)
{
    if (!f.sparse) return 0;
    std::vector<seeds::Size> q;
    for (int k = 0; k < K; k++) q.push_back(seeds::Size{sz[k].first, sz[k].second});
    const sparse::Layout L = sparse::layout(q);
    return pad4((size_t)q[0].r * q[0].c) + (L.total - L.t1);
}

// Uploads the host map D and fills Dp[0..K): the dense form as it always did, the sparse one through `extra`.
template <class Sizes>
int build_d_pyramid(const Form &f, hipStream_t s, const float *D, const Sizes &sz, int K, float *const *Dp, float *extra)
{
    const size_t n0 = (size_t)sz[0].first * sz[0].second;
    if (!f.sparse) {
        HIPCHK(hipMemcpy(Dp[0], D, n0 * sizeof(float), hipMemcpyHostToDevice));
        for (int k = 1; k < K; k++)
            RC(pdeip_pyr_resize_dev(s, Dp[k - 1], sz[k - 1].first, sz[k - 1].second, 1, sz[k].first, sz[k].second, 1, Dp[k]));
        return PDEIP_OK;
    }
    std::vector<int> rc;
    for (int k = 0; k < K; k++) {
        rc.push_back(sz[k].first);
        rc.push_back(sz[k].second);
    }
    float *t1 = extra + pad4(n0), *t2 = t1 + (K > 1 ? pad4(n0) : 0);
    HIPCHK(hipMemcpy(extra, D, n0 * sizeof(float), hipMemcpyHostToDevice));
    return sparse_pyramid_dev(s, extra, rc.data(), K, Dp, t1, t2);
}

} // namespace

extern "C" int pdeip_seg_sizes_dev(void *stream, const float *PHI, int nrows, int ncols, int S, int *sizes_out)
{
    const char *who = "pdeip_seg_sizes_dev";
    NONNULL(who, PHI); NONNULL(who, sizes_out);
    RC(check_planes(who, nrows, ncols, S));
    double *psum = nullptr;
    int *part = nullptr;
    RC(stage_ws(nrows * ncols, S, &psum, &part));
    RC(launch_sizes(static_cast<hipStream_t>(stream), PHI, nrows * ncols, S, part, sizes_out));
    tls.last_launches = 2;
    return PDEIP_OK;
}

extern "C" int pdeip_seg_variance_dev(void *stream, const float *PHI, const float *dist, int nrows, int ncols, int S, double minCOV, double dist_cap,
                                      double *cov_out, int *n_out)
{
    const char *who = "pdeip_seg_variance_dev";
    NONNULL(who, PHI); NONNULL(who, dist); NONNULL(who, cov_out);
    RC(check_planes(who, nrows, ncols, S));
    if (!std::isfinite(minCOV) || minCOV <= 0.0) return set_err(PDEIP_ERR_ARG, "%s: minCOV must be finite and > 0", who);
    if (std::isnan(dist_cap)) dist_cap = std::numeric_limits<double>::infinity();
    double *psum = nullptr;
    int *pcnt = nullptr;
    RC(stage_ws(nrows * ncols, S, &psum, &pcnt));
    RC(launch_variance(static_cast<hipStream_t>(stream), PHI, dist, nrows * ncols, S, minCOV, dist_cap, psum, pcnt, cov_out, n_out));
    tls.last_launches = 2;
    return PDEIP_OK;
}

extern "C" int pdeip_seg_data_dev(void *stream, const float *dist, const float *PHI, const float *DH, const double *cov, int nrows, int ncols, int S,
                                  int strategy, float *DATA_out, double *P_out)
{
    const char *who = "pdeip_seg_data_dev";
    NONNULL(who, dist); NONNULL(who, PHI); NONNULL(who, DH); NONNULL(who, cov); NONNULL(who, DATA_out);
    RC(check_planes(who, nrows, ncols, S));
    RC(check_strategy(who, strategy));
    if (DATA_out == dist || DATA_out == PHI || DATA_out == DH) return set_err(PDEIP_ERR_ARG, "%s: DATA_out must not alias an input", who);
    RC(launch_data(static_cast<hipStream_t>(stream), dist, PHI, DH, cov, nrows * ncols, S, strategy, DATA_out, P_out));
    tls.last_launches = 1;
    return PDEIP_OK;
}

extern "C" int pdeip_seg_label_dev(void *stream, const float *PHI, int nrows, int ncols, int S, int *SEG_out)
{
    const char *who = "pdeip_seg_label_dev";
    NONNULL(who, PHI); NONNULL(who, SEG_out);
    RC(check_planes(who, nrows, ncols, S));
    const int npix = nrows * ncols;
    hipLaunchKernelGGL(k_seg_label, dim3((unsigned)tiles_of(npix)), dim3(SG_BLOCK), 0, static_cast<hipStream_t>(stream), PHI, npix, S, SEG_out);
    HIPCHK(hipGetLastError());
    tls.last_launches = 1;
    return PDEIP_OK;
}

extern "C" int pdeip_seg_label(const float *PHI, int nrows, int ncols, int S, int *SEG_out)
{
    const char *who = "pdeip_seg_label";
    NONNULL(who, PHI); NONNULL(who, SEG_out);
    RC(check_planes(who, nrows, ncols, S));
    RC(use_device());
    const size_t n = (size_t)nrows * ncols;
    float *ar = nullptr;
    RC(ws_get(WS_ARENA, (pad4(n * S) + pad4(n)) * sizeof(float), &ar));
    int *dSeg = reinterpret_cast<int *>(ar + pad4(n * S));
    HIPCHK(hipMemcpy(ar, PHI, n * S * sizeof(float), hipMemcpyHostToDevice));
    RC(pdeip_seg_label_dev(nullptr, ar, nrows, ncols, S, dSeg));
    HIPCHK(hipMemcpy(SEG_out, dSeg, n * sizeof(int), hipMemcpyDeviceToHost));
    return PDEIP_OK;
}

// ---- one scale: `iterations` competition iterations, resident ----------------------------------------------------------------------
extern "C" int pdeip_seg_competition_level_dev(void *stream, const float *PHI, const float *D, int nrows, int ncols, int S, int order, int strategy,
                                               double minCOV, float ransac_cset, int iterations, double srem_thr, unsigned long long seed,
                                               unsigned long long *fit_counter, const pdeip_seg_params *prm, int *S_out, float *PHI_out,
                                               float *surf_out, int *kept_out, double *cov_out)
{
    const char *who = "pdeip_seg_competition_level_dev";
    tls.err[0] = '\0'; // a call that succeeds leaves pdeip_last_error() empty
    NONNULL(who, PHI); NONNULL(who, D); NONNULL(who, S_out); NONNULL(who, PHI_out); NONNULL(who, surf_out); NONNULL(who, kept_out);
    const SegPrm p = seg_resolve(prm);
    RC(check_level(who, nrows, ncols, S, order, strategy, minCOV, ransac_cset, iterations, srem_thr, p));
    if (PHI_out == PHI) return set_err(PDEIP_ERR_ARG, "%s: PHI_out must not alias PHI", who);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int npix = nrows * ncols, ncoef = order == 1 ? 3 : 6, tiles = tiles_of(npix);
    const size_t np = (size_t)S * tiles, nS = pad4((size_t)S * npix);
    const float nu = (float)(p.gamma_coef * std::pow((double)nrows * (double)ncols, 0.7));
    const double remove_below = srem_thr * (double)nrows * (double)ncols;

    // workspace: the doubles first (8-byte aligned: a hipMalloc'd base, every offset a multiple of 4 floats)
    float *ws = nullptr;
    const size_t nDbl = pad4(2 * (np + (size_t)S));
    RC(ws_get(WS_SEG, (nDbl + 2 * pad4(np) + pad4((size_t)S) + pad4((size_t)S * ncoef) + pad4((size_t)npix) + 6 * nS) * sizeof(float), &ws));
    double *psum = reinterpret_cast<double *>(ws), *cov = psum + np;
    int *pcnt = reinterpret_cast<int *>(ws + nDbl), *part = pcnt + pad4(np), *sizes = part + pad4(np);
    float *models = reinterpret_cast<float *>(sizes + pad4((size_t)S));
    float *Dfill = models + pad4((size_t)S * ncoef);
    float *cur = Dfill + pad4((size_t)npix), *nxt = cur + nS, *DATA = nxt + nS, *DH = DATA + nS, *GRAD = DH + nS, *DIST = GRAD + nS;
    int *host_sizes = nullptr;
    RC(pinned_sizes(S, &host_sizes));

    const bool fit_chains = env_int("PDEIP_SEG_FIT_CHAINS", 0) != 0; // 1: one single-fit chain per segment (the A/B switch of tools/time_segmentation.py)
    int launches = 0;
    RC(copy_d2d(s, cur, PHI, (size_t)S * npix));
    const float *Dsrc = D;
    if (!std::isnan(p.nan_fill)) {
        hipLaunchKernelGGL(k_seg_nanfill, dim3((unsigned)tiles), dim3(SG_BLOCK), 0, s, D, npix, p.nan_fill, Dfill);
        HIPCHK(hipGetLastError());
        Dsrc = Dfill;
        launches++;
    }
    HIPCHK(hipMemsetAsync(models, 0, (size_t)S * ncoef * sizeof(float), s));
    HIPCHK(hipMemsetAsync(cov, 0, (size_t)S * sizeof(double), s));

    std::vector<int> kept((size_t)S);
    for (int k = 0; k < S; k++) kept[k] = k;
    int live = S;
    bool recalc = false;
    unsigned long long fit = fit_counter ? *fit_counter : 0ull;
    for (int it = 1; it <= iterations; it++) {
        // 1. sizes, read back once (the removal decides the shapes of everything after it)
        RC(launch_sizes(s, cur, npix, live, part, sizes));
        HIPCHK(hipMemcpyAsync(host_sizes, sizes, (size_t)live * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        launches += 2;
        int n_kept = 0;
        for (int k = 0; k < live; k++) {
            if ((double)host_sizes[k] < remove_below) continue;
            if (n_kept != k) { // survivors move down in order: the destination plane is always below its source
                RC(copy_d2d(s, cur + (size_t)n_kept * npix, cur + (size_t)k * npix, (size_t)npix));
                launches++;
            }
            kept[n_kept++] = kept[k];
        }
        if (n_kept != live) {
            live = n_kept;
            recalc = true;
            if (live == 0) break;
            HIPCHK(hipMemsetAsync(models, 0, (size_t)S * ncoef * sizeof(float), s)); // ALL the models, as the .m does
        }
        // 2. the terms
        if ((it & 1) || recalc) {
            RC(pdeip_cv_terms_dev(s, cur, nrows, ncols, live, p.c0, p.c1, p.dh_floor, DH, GRAD));
            launches += 1;
            if (!fit_chains && live <= 65535) { // every live segment's fit in one chain: segment k draws from seed + 65536*(fit + k)
                RC(pdeip_surface_fit_masked_batch_dev(s, cur, Dsrc, nrows, ncols, live, order, models, p.err_thr, ransac_cset, 10,
                                                      seed + 65536ull * fit, 65536ull, models, DIST, nullptr));
                launches += tls.last_launches;
                fit += (unsigned long long)live;
            } else {
                for (int k = 0; k < live; k++) {
                    float *M = models + (size_t)k * ncoef;
                    RC(pdeip_surface_fit_masked_dev(s, cur + (size_t)k * npix, Dsrc, nrows, ncols, order, M, p.err_thr, ransac_cset, 10, nullptr,
                                                    seed + 65536ull * fit, M, DIST + (size_t)k * npix, nullptr));
                    launches += tls.last_launches;
                    fit++;
                }
            }
            RC(launch_variance(s, cur, DIST, npix, live, minCOV, p.dist_cap, psum, pcnt, cov, nullptr));
            RC(launch_data(s, DIST, cur, DH, cov, npix, live, strategy, DATA, nullptr));
            launches += 3;
            recalc = false;
        }
        // 3. the step
        RC(pdeip_cv_solver_dev(s, cur, DATA, DH, GRAD, nrows, ncols, live, 1.0f, nu, nxt));
        launches += tls.last_launches;
        std::swap(cur, nxt);
    }
    if (fit_counter) *fit_counter = fit;
    *S_out = live;
    for (int k = 0; k < live; k++) kept_out[k] = kept[k];
    if (live > 0) {
        RC(copy_d2d(s, PHI_out, cur, (size_t)live * npix));
        RC(copy_d2d(s, surf_out, models, (size_t)live * ncoef));
        if (cov_out) RC(copy_d2d(s, reinterpret_cast<float *>(cov_out), reinterpret_cast<const float *>(cov), 2 * (size_t)live));
        launches += 3;
    }
    tls.last_launches = launches;
    return PDEIP_OK;
}

extern "C" int pdeip_seg_competition_level(const float *PHI, const float *D, int nrows, int ncols, int S, int order, int strategy, double minCOV,
                                           float ransac_cset, int iterations, double srem_thr, unsigned long long seed,
                                           unsigned long long *fit_counter, const pdeip_seg_params *prm, int *S_out, float *PHI_out,
                                           float *surf_out, int *kept_out, double *cov_out)
{
    const char *who = "pdeip_seg_competition_level";
    tls.err[0] = '\0'; // a call that succeeds leaves pdeip_last_error() empty
    NONNULL(who, PHI); NONNULL(who, D); NONNULL(who, S_out); NONNULL(who, PHI_out); NONNULL(who, surf_out); NONNULL(who, kept_out);
    const SegPrm p = seg_resolve(prm);
    RC(check_level(who, nrows, ncols, S, order, strategy, minCOV, ransac_cset, iterations, srem_thr, p));
    RC(use_device());
    const size_t n = (size_t)nrows * ncols, nS = pad4(n * S);
    const int ncoef = order == 1 ? 3 : 6;
    float *ar = nullptr;
    RC(ws_get(WS_ARENA, (pad4(2 * (size_t)S) + 2 * nS + pad4(n) + pad4((size_t)S * ncoef)) * sizeof(float), &ar));
    double *dCov = reinterpret_cast<double *>(ar);
    float *dP = ar + pad4(2 * (size_t)S), *dO = dP + nS, *dD = dO + nS, *dM = dD + pad4(n);
    HIPCHK(hipMemcpy(dP, PHI, n * S * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dD, D, n * sizeof(float), hipMemcpyHostToDevice));
    RC(pdeip_seg_competition_level_dev(nullptr, dP, dD, nrows, ncols, S, order, strategy, minCOV, ransac_cset, iterations, srem_thr, seed, fit_counter,
                                       prm, S_out, dO, dM, kept_out, dCov));
    const int live = *S_out;
    if (live > 0) {
        HIPCHK(hipMemcpy(PHI_out, dO, n * live * sizeof(float), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(surf_out, dM, (size_t)live * ncoef * sizeof(float), hipMemcpyDeviceToHost));
        if (cov_out) HIPCHK(hipMemcpy(cov_out, dCov, (size_t)live * sizeof(double), hipMemcpyDeviceToHost));
    }
    return PDEIP_OK;
}

// ---- regionCompetition(): the D pyramid, the visits [1..K, K..1], PHI carried from visit to visit --------------------------------
namespace {

int region_competition(const char *who, const Form &form, const float *D, const float *PHI, int nrows, int ncols, int S, int order, int strategy,
                       double sigmaLim, float ransac_cset, int iterations, double srem_thr, double scl_factor, double rc_scl,
                       unsigned long long seed, const pdeip_seg_params *prm, int *S_out, float *PHI_out, float *surf_out, int *kept_out)
{
    tls.err[0] = '\0'; // a call that succeeds leaves pdeip_last_error() empty
    NONNULL(who, D); NONNULL(who, PHI); NONNULL(who, S_out); NONNULL(who, PHI_out); NONNULL(who, surf_out); NONNULL(who, kept_out);
    const SegPrm p = seg_resolve(prm, form.sparse);
    // what every level call of this run resolves to: the dense form hands the caller's struct on as it is
    const pdeip_seg_params full{p.c0, p.c1, p.dh_floor, p.err_thr, p.gamma_coef, p.dist_cap, p.nan_fill};
    const pdeip_seg_params *level_prm = form.sparse ? &full : prm;
    RC(check_level(who, nrows, ncols, S, order, strategy, sigmaLim, ransac_cset, iterations, srem_thr, p));
    if (!(scl_factor > 0.0 && scl_factor < 1.0)) return set_err(PDEIP_ERR_ARG, "%s: scl_factor must lie in (0, 1) (got %g)", who, scl_factor);
    if (!(rc_scl > 0.0) || !std::isfinite(rc_scl)) return set_err(PDEIP_ERR_ARG, "%s: rc_scl must be finite and > 0 (got %g)", who, rc_scl);
    if (nrows < 3 || ncols < 3) return set_err(PDEIP_ERR_ARG, "%s: D must be at least 3x3 (got %dx%d)", who, nrows, ncols);
    // scales: size(imresize(D, scl_factor)) = ceil(size * scl_factor) while both sides stay >= rc_scl x the original
    std::vector<std::pair<int, int>> sz{{nrows, ncols}};
    for (;;) {
        const int r = (int)std::ceil(sz.back().first * scl_factor), c = (int)std::ceil(sz.back().second * scl_factor);
        if (!((double)r >= nrows * rc_scl && (double)c >= ncols * rc_scl) || r < 3 || c < 3) break;
        if (r == sz.back().first && c == sz.back().second) break; // a size that no longer shrinks ends the pyramid
        sz.push_back({r, c});
    }
    const int K = (int)sz.size(), ncoef = order == 1 ? 3 : 6;
    RC(use_device());
    const size_t n0 = (size_t)nrows * ncols, nS = pad4(n0 * S);
    size_t nD = 0;
    for (auto &q : sz) nD += pad4((size_t)q.first * q.second);
    float *ws = nullptr;
    RC(ws_get(WS_SEG_RC, (nD + 2 * nS + pad4((size_t)S * ncoef) + pyramid_extra(form, sz, K)) * sizeof(float), &ws));
    std::vector<float *> Dp((size_t)K);
    float *at = ws;
    for (int k = 0; k < K; k++) {
        Dp[k] = at;
        at += pad4((size_t)sz[k].first * sz[k].second);
    }
    float *A = at, *B = A + nS, *dM = B + nS;
    RC(build_d_pyramid(form, nullptr, D, sz, K, Dp.data(), dM + pad4((size_t)S * ncoef)));
    HIPCHK(hipMemcpy(A, PHI, n0 * S * sizeof(float), hipMemcpyHostToDevice));

    std::vector<int> visits;
    for (int k = 0; k < K; k++) visits.push_back(k);
    for (int k = K - 1; k >= 0; k--) visits.push_back(k);
    std::vector<int> kept((size_t)S), kv((size_t)S);
    for (int k = 0; k < S; k++) kept[k] = k;
    int live = S;
    unsigned long long fit = 0;
    for (size_t v = 0; v < visits.size(); v++) {
        const int k = visits[v], r = sz[k].first, c = sz[k].second;
        int out = 0;
        RC(pdeip_seg_competition_level_dev(nullptr, A, Dp[k], r, c, live, order, strategy, sigmaLim, ransac_cset, iterations, srem_thr, seed, &fit,
                                           level_prm, &out, B, dM, kv.data(), nullptr));
        for (int i = 0; i < out; i++) kept[i] = kept[kv[i]];
        live = out;
        if (live == 0) break;
        if (v + 1 < visits.size()) {
            const int kn = visits[v + 1];
            RC(pdeip_pyr_resize_dev(nullptr, B, r, c, live, sz[kn].first, sz[kn].second, 1, A));
        }
    }
    *S_out = live;
    for (int i = 0; i < live; i++) kept_out[i] = kept[i];
    if (live > 0) {
        HIPCHK(hipMemcpy(PHI_out, B, n0 * live * sizeof(float), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(surf_out, dM, (size_t)live * ncoef * sizeof(float), hipMemcpyDeviceToHost));
    } else {
        HIPCHK(hipDeviceSynchronize());
    }
    return PDEIP_OK;
}

} // namespace

extern "C" int pdeip_region_competition(const float *D, const float *PHI, int nrows, int ncols, int S, int order, int strategy, double sigmaLim,
                                        float ransac_cset, int iterations, double srem_thr, double scl_factor, double rc_scl, unsigned long long seed,
                                        const pdeip_seg_params *prm, int *S_out, float *PHI_out, float *surf_out, int *kept_out)
{
    return region_competition("pdeip_region_competition", DENSE_FORM, D, PHI, nrows, ncols, S, order, strategy, sigmaLim, ransac_cset, iterations,
                              srem_thr, scl_factor, rc_scl, seed, prm, S_out, PHI_out, surf_out, kept_out);
}

extern "C" int pdeip_region_competition_sparse(const float *D, const float *PHI, int nrows, int ncols, int S, int order, int strategy,
                                               double sigmaLim, float ransac_cset, int iterations, double srem_thr, double scl_factor,
                                               double rc_scl, unsigned long long seed, const pdeip_seg_params *prm, int *S_out, float *PHI_out,
                                               float *surf_out, int *kept_out)
{
    return region_competition("pdeip_region_competition_sparse", SPARSE_FORM, D, PHI, nrows, ncols, S, order, strategy, sigmaLim, ransac_cset,
                              iterations, srem_thr, scl_factor, rc_scl, seed, prm, S_out, PHI_out, surf_out, kept_out);
}

// ---- generateSeeds() (DispSegmentation.m:203-443): seed after seed, each grown over the visits [1..K, K..1] -----------------------
namespace {

int check_seeds(const char *who, int nrows, int ncols, int order, double sigmaLim, const double *cset_vect, int n_cset, int iterations, int n_seeds,
                double scl_factor, double pyr_scl)
{
    char buf[160];
    const char *bad = seeds::check_args(buf, sizeof buf, nrows, ncols, order, sigmaLim, cset_vect, n_cset, iterations, n_seeds, scl_factor, pyr_scl);
    return bad ? set_err(PDEIP_ERR_ARG, "%s: %s", who, bad) : PDEIP_OK;
}

int generate_seeds(const char *who, const Form &form, const float *D, const float *AA, int nrows, int ncols, int order, double sigmaLim,
                   const double *cset_vect, int n_cset, int iterations, int n_seeds, double scl_factor, double pyr_scl, unsigned long long seed,
                   unsigned long long *fit_counter, const pdeip_seeds_params *prm, pdeip_seeds_trace *trace, int *S_out, float *PHI_out,
                   float *surf_out)
{
    tls.err[0] = '\0'; // a call that succeeds leaves pdeip_last_error() empty
    NONNULL(who, D); NONNULL(who, S_out); NONNULL(who, PHI_out); NONNULL(who, surf_out);
    RC(check_seeds(who, nrows, ncols, order, sigmaLim, cset_vect, n_cset, iterations, n_seeds, scl_factor, pyr_scl));
    const seeds::Prm p = sparse::resolve(form.sparse ? sparse::seeds_defaults() : sparse::dense_seeds_defaults(), prm ? &prm->dist_cap : nullptr,
                                         prm ? &prm->nan_fill : nullptr, prm ? &prm->mincov_gate : nullptr);
    const std::vector<seeds::Size> sz = seeds::scale_sizes(nrows, ncols, scl_factor, pyr_scl);
    const int K = (int)sz.size(), ncoef = order == 1 ? 3 : 6;
    const bool fill = !std::isnan(p.nan_fill);
    RC(use_device());
    hipStream_t s = nullptr;
    const size_t n0 = (size_t)nrows * ncols, nP = pad4(n0);
    size_t nD = 0;
    for (auto &q : sz) nD += pad4((size_t)q.r * q.c);
    // workspace: cov (a double) first, then the count, the model, the pyramids of D, of D without NaNs and of AA, six planes
    float *ws = nullptr;
    std::vector<std::pair<int, int>> szp;
    for (auto &q : sz) szp.push_back({q.r, q.c});
    RC(ws_get(WS_SEEDS, (4 + 4 + 8 + (fill ? 3 : 2) * nD + 6 * nP + pyramid_extra(form, szp, K)) * sizeof(float), &ws));
    double *cov = reinterpret_cast<double *>(ws);
    int *cnt = reinterpret_cast<int *>(ws + 4);
    float *M = ws + 8, *at = M + 8;
    std::vector<float *> Dp((size_t)K), Df((size_t)K), Ap((size_t)K);
    for (int pass = 0; pass < (fill ? 3 : 2); pass++)
        for (int k = 0; k < K; k++) {
            (pass == 0 ? Dp : pass == 1 ? Ap : Df)[(size_t)k] = at;
            at += pad4((size_t)sz[k].r * sz[k].c);
        }
    float *cur = at, *nxt = cur + nP, *DATA = nxt + nP, *DH = DATA + nP, *GRAD = DH + nP, *DIST = GRAD + nP;
    int *host_cnt = nullptr;
    RC(pinned_sizes(4, &host_cnt)); // the count in word 0, the variance of v = K (a double) in words 2-3 of the level call's pinned block
    double *host_cov = reinterpret_cast<double *>(host_cnt + 2);
    double *psum = nullptr;
    int *pcnt = nullptr;

    RC(build_d_pyramid(form, s, D, szp, K, Dp.data(), DIST + nP));
    {
        std::vector<float> a(n0, 1.0f); // AA{1}: all ones, or the caller's with its NaNs counted as 0
        if (AA)
            for (size_t i = 0; i < n0; i++) a[i] = AA[i] != AA[i] ? 0.0f : AA[i];
        HIPCHK(hipMemcpy(Ap[0], a.data(), n0 * sizeof(float), hipMemcpyHostToDevice));
    }
    for (int k = 0; k < K; k++) {
        if (!fill) { Df[(size_t)k] = Dp[(size_t)k]; continue; }
        const int npix = sz[k].r * sz[k].c;
        hipLaunchKernelGGL(k_seg_nanfill, dim3((unsigned)tiles_of(npix)), dim3(SG_BLOCK), 0, s, Dp[k], npix, p.nan_fill, Df[k]);
        HIPCHK(hipGetLastError());
    }

    if (trace) trace->n_counts = trace->n_largest = 0;
    const size_t nK = (size_t)sz[K - 1].r * sz[K - 1].c;
    double gamma = form.gamma0;
    unsigned long long fit = fit_counter ? *fit_counter : 0ull;
    int S = 0;
    for (int sd = 0; sd < n_seeds; sd++) {
        for (int k = 1; k < K; k++) RC(pdeip_pyr_resize_dev(s, Ap[k - 1], sz[k - 1].r, sz[k - 1].c, 1, sz[k].r, sz[k].c, 1, Ap[k]));
        double minCOV = sigmaLim;
        hipLaunchKernelGGL(k_seeds_init, dim3((unsigned)tiles_of((int)n0)), dim3(SG_BLOCK), 0, s, nrows, ncols, cur);
        HIPCHK(hipGetLastError());
        bool empty = false;
        for (int v = 0; v < 2 * K; v++) {
            const int k = seeds::visit_scale(v, K), r = sz[k].r, c = sz[k].c, npix = r * c;
            const dim3 grid((unsigned)tiles_of(npix)), blk(SG_BLOCK);
            RC(stage_ws(npix, 1, &psum, &pcnt));
            if (v == 0) hipLaunchKernelGGL(k_seeds_exclude, grid, blk, 0, s, Ap[k], npix, seeds::INCLUDE_ABOVE, -1.0f, cur);
            bool have_model = false; // H1eq = [] (:279)
            if (v == K) { // once per seed only the biggest connected element survives (:282-298)
                RC(pdeip_largest_component_dev(s, cur, r, c, 8, 5.0f, -5.0f, cur, nullptr, nullptr));
                if (trace && trace->largest) {
                    HIPCHK(hipMemcpyAsync(trace->largest + (size_t)trace->n_largest * nK, cur, nK * sizeof(float), hipMemcpyDeviceToHost, s));
                    trace->n_largest++;
                }
            }
            const float nu = seeds::nu_of(gamma, r, c);
            for (int it = 1; it <= iterations; it++) {
                // the count, read back once: it decides whether the seed goes on
                RC(launch_sizes(s, cur, npix, 1, pcnt, cnt));
                HIPCHK(hipMemcpyAsync(host_cnt, cnt, sizeof(int), hipMemcpyDeviceToHost, s));
                HIPCHK(hipStreamSynchronize(s));
                if (trace && trace->counts && trace->n_counts < trace->counts_cap) trace->counts[trace->n_counts] = *host_cnt;
                if (trace) trace->n_counts++;
                if (*host_cnt < seeds::EMPTY_BELOW) {
                    empty = true;
                    break;
                }
                RC(pdeip_surface_fit_masked_dev(s, cur, Df[k], r, c, order, have_model ? M : nullptr, seeds::ERR_THR,
                                                (float)seeds::rcons(cset_vect, n_cset, it, v), seeds::riter(it, v), nullptr, seed + 65536ull * fit, M,
                                                DIST, nullptr));
                fit++;
                have_model = true;
                RC(launch_variance(s, cur, DIST, npix, 1, minCOV, p.dist_cap, psum, pcnt, cov, nullptr));
                RC(pdeip_cv_terms_dev(s, cur, r, c, 1, 1.0f, 1.0f, std::numeric_limits<float>::quiet_NaN(), DH, GRAD));
                RC(launch_data(s, DIST, cur, DH, cov, npix, 1, PDEIP_SEG_INVERSE, DATA, nullptr));
                hipLaunchKernelGGL(k_seeds_exclude, grid, blk, 0, s, Ap[k], npix, seeds::INCLUDE_ABOVE, -2.0f, DATA);
                HIPCHK(hipGetLastError());
                RC(pdeip_cv_solver_dev(s, cur, DATA, DH, GRAD, r, c, 1, 1.0f, nu, nxt));
                std::swap(cur, nxt);
            }
            if (empty) {
                gamma *= seeds::GAMMA_SHRINK; // persists over the remaining seeds (:402-405)
                break;
            }
            if (v == K && iterations > 0) { // minCOV = the unfloored variance of the last iteration: its H1 (nxt) and distD (:408-412)
                RC(launch_variance(s, nxt, DIST, npix, 1, -std::numeric_limits<double>::infinity(), p.dist_cap, psum, pcnt, cov, nullptr));
                HIPCHK(hipMemcpyAsync(host_cov, cov, sizeof(double), hipMemcpyDeviceToHost, s));
                HIPCHK(hipStreamSynchronize(s));
                if (*host_cov > p.mincov_gate) minCOV = *host_cov; // a NaN never exceeds the gate
            }
            if (v + 1 < 2 * K) {
                const int kn = seeds::visit_scale(v + 1, K);
                RC(pdeip_pyr_resize_dev(s, cur, r, c, 1, sz[kn].r, sz[kn].c, 1, nxt));
                std::swap(cur, nxt);
            }
        }
        if (empty) continue;
        HIPCHK(hipMemcpyAsync(PHI_out + (size_t)S * n0, cur, n0 * sizeof(float), hipMemcpyDeviceToHost, s));
        if (iterations > 0) HIPCHK(hipMemcpyAsync(surf_out + (size_t)S * ncoef, M, (size_t)ncoef * sizeof(float), hipMemcpyDeviceToHost, s));
        else std::fill(surf_out + (size_t)S * ncoef, surf_out + (size_t)(S + 1) * ncoef, std::numeric_limits<float>::quiet_NaN()); // no fit: no model
        S++;
        hipLaunchKernelGGL(k_seeds_allowed, dim3((unsigned)tiles_of((int)n0)), dim3(SG_BLOCK), 0, s, cur, (int)n0, Ap[0]);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(s));
    if (fit_counter) *fit_counter = fit;
    *S_out = S;
    return PDEIP_OK;
}

} // namespace

extern "C" int pdeip_generate_seeds(const float *D, const float *AA, int nrows, int ncols, int order, double sigmaLim, const double *cset_vect,
                                    int n_cset, int iterations, int n_seeds, double scl_factor, double pyr_scl, unsigned long long seed,
                                    unsigned long long *fit_counter, const pdeip_seeds_params *prm, pdeip_seeds_trace *trace, int *S_out,
                                    float *PHI_out, float *surf_out)
{
    return generate_seeds("pdeip_generate_seeds", DENSE_FORM, D, AA, nrows, ncols, order, sigmaLim, cset_vect, n_cset, iterations, n_seeds, scl_factor,
                          pyr_scl, seed, fit_counter, prm, trace, S_out, PHI_out, surf_out);
}

extern "C" int pdeip_generate_seeds_sparse(const float *D, const float *AA, int nrows, int ncols, int order, double sigmaLim,
                                           const double *cset_vect, int n_cset, int iterations, int n_seeds, double scl_factor, double pyr_scl,
                                           unsigned long long seed, unsigned long long *fit_counter, const pdeip_seeds_params *prm,
                                           pdeip_seeds_trace *trace, int *S_out, float *PHI_out, float *surf_out)
{
    return generate_seeds("pdeip_generate_seeds_sparse", SPARSE_FORM, D, AA, nrows, ncols, order, sigmaLim, cset_vect, n_cset, iterations, n_seeds,
                          scl_factor, pyr_scl, seed, fit_counter, prm, trace, S_out, PHI_out, surf_out);
}

// ---- [PHI SEG SParam] = DispSegmentation(Din, param) (DispSegmentation.m:31-198) ------------------------------------------------
// The sparse driver (DispSegmentationSparse.m:42-202) is the same sequence of stages with its own defaults, Din's NaNs left in place
// and the sparse stage calls.
namespace {

int disp_segmentation(const char *who, bool sparse_form, const float *Din, int nrows, int ncols, const float *PHIin, int S_in, const float *AA,
                      const pdeip_dispseg_params *prm, unsigned long long seed, int *S_out, float *PHI_out, int *SEG_out, float *surf_out)
{
    tls.err[0] = '\0';
    NONNULL(who, Din); NONNULL(who, S_out); NONNULL(who, PHI_out); NONNULL(who, SEG_out); NONNULL(who, surf_out);
    seeds::DriverPrm p = sparse_form ? sparse::driver_defaults() : seeds::driver_defaults();
    if (prm) {
        if (!std::isnan(prm->srem_thr)) p.srem_thr = prm->srem_thr;
        if (!std::isnan(prm->scl_factor)) p.scl_factor = prm->scl_factor;
        if (!std::isnan(prm->gen_scl)) p.gen_scl = prm->gen_scl;
        if (!std::isnan(prm->rc_scl)) p.rc_scl = prm->rc_scl;
        if (!std::isnan(prm->ransac_min_cset)) p.ransac_min_cset = prm->ransac_min_cset;
        if (!std::isnan(prm->ransac_max_cset)) p.ransac_max_cset = prm->ransac_max_cset;
        if (prm->polyorder != 0) p.polyorder = prm->polyorder;
        if (prm->seeds != 0) p.seeds = prm->seeds;
        if (prm->ransac_cset_cycles != 0) p.ransac_cset_cycles = prm->ransac_cset_cycles;
    }
    {
        char buf[160];
        const char *bad = seeds::check_driver(buf, sizeof buf, p);
        if (bad) return set_err(PDEIP_ERR_ARG, "%s: %s", who, bad);
    }
    if (PHIin && S_in < 1) return set_err(PDEIP_ERR_ARG, "%s: PHIin given with S_in = %d", who, S_in);
    const std::vector<double> cset = seeds::cset_vector(p.ransac_min_cset, p.ransac_max_cset, p.ransac_cset_cycles);
    const int cap = PHIin ? S_in + 1 : 2 * p.seeds;
    RC(check_seeds(who, nrows, ncols, p.polyorder, 0.7, cset.data(), (int)cset.size(), 20, std::max(cap, 1), p.scl_factor, p.gen_scl));
    const SegPrm stage_prm = seg_resolve(nullptr, sparse_form);
    RC(check_level(who, nrows, ncols, cap, p.polyorder, PDEIP_SEG_INVERSE, 1.0, (float)p.ransac_max_cset, 20, p.srem_thr, stage_prm));
    const auto compete_call = sparse_form ? pdeip_region_competition_sparse : pdeip_region_competition;
    const auto seeds_call = sparse_form ? pdeip_generate_seeds_sparse : pdeip_generate_seeds;

    const size_t n0 = (size_t)nrows * ncols;
    const int ncoef = p.polyorder == 1 ? 3 : 6;
    std::vector<float> Dz(Din, Din + n0), A(n0), P((size_t)cap * n0), Q((size_t)cap * n0);
    std::vector<int> kept((size_t)cap);
    if (!sparse_form)
        for (auto &d : Dz)
            if (d != d) d = 0.0f; // we don't like NaNs (:61); the sparse driver filters them inside its stages (:63-64)
    int live = 0, stage = 0;
    *S_out = 0;
    auto compete = [&](double sigmaLim, int iterations) -> int { // P -> P
        int out = 0;
        RC(compete_call(Dz.data(), P.data(), nrows, ncols, live, p.polyorder, PDEIP_SEG_INVERSE, sigmaLim, (float)p.ransac_max_cset,
                                    iterations, p.srem_thr,
                         p.scl_factor, p.rc_scl, seeds::stage_seed(seed, stage++), nullptr, &out, Q.data(), surf_out, kept.data()));
        live = out;
        std::swap(P, Q);
        return PDEIP_OK;
    };
    auto more_seeds = [&](double sigmaLim, const float *allowed, int n, double pyr_scl) -> int { // appends to P
        int out = 0;
        RC(seeds_call(Dz.data(), allowed, nrows, ncols, p.polyorder, sigmaLim, cset.data(), (int)cset.size(), 20, n, p.scl_factor, pyr_scl,
                                seeds::stage_seed(seed, stage++), nullptr, nullptr, nullptr, &out, P.data() + (size_t)live * n0,
                                surf_out + (size_t)live * ncoef));
        live += out;
        return PDEIP_OK;
    };
    auto uncovered = [&]() { // sum(PHI > 0, 3) == 0
        for (size_t i = 0; i < n0; i++) {
            bool any = false;
            for (int k = 0; k < live && !any; k++) any = P[(size_t)k * n0 + i] > 0.0f;
            A[i] = any ? 0.0f : 1.0f;
        }
    };
    if (!PHIin) {
        const float *allowed = nullptr; // param.AA == 1; an empty AA allows everything
        if (AA) {
            for (size_t i = 0; i < n0; i++) A[i] = AA[i] == 1.0f ? 1.0f : 0.0f;
            allowed = A.data();
        }
        RC(more_seeds(0.7, allowed, p.seeds, p.gen_scl));
        if (live == 0) return PDEIP_OK;
        if (p.seeds != 1) {
            RC(compete(1.5, 30));
            if (live == 0) return PDEIP_OK;
            uncovered();
            RC(more_seeds(1.2, A.data(), p.seeds, p.rc_scl));
            RC(compete(1.5, 20));
        }
    } else {
        std::copy(PHIin, PHIin + (size_t)S_in * n0, P.begin());
        live = S_in;
        RC(compete(1.0, 20));
        if (live == 0) return PDEIP_OK;
        uncovered();
        RC(more_seeds(1.2, A.data(), 1, p.rc_scl));
        RC(compete(2.0, 20));
    }
    if (live == 0) return PDEIP_OK;
    std::copy(P.begin(), P.begin() + (size_t)live * n0, PHI_out);
    RC(pdeip_seg_label(PHI_out, nrows, ncols, live, SEG_out));
    *S_out = live;
    return PDEIP_OK;
}

} // namespace

extern "C" int pdeip_disp_segmentation(const float *Din, int nrows, int ncols, const float *PHIin, int S_in, const float *AA,
                                       const pdeip_dispseg_params *prm, unsigned long long seed, int *S_out, float *PHI_out, int *SEG_out,
                                       float *surf_out)
{
    return disp_segmentation("pdeip_disp_segmentation", false, Din, nrows, ncols, PHIin, S_in, AA, prm, seed, S_out, PHI_out, SEG_out, surf_out);
}

extern "C" int pdeip_disp_segmentation_sparse(const float *Din, int nrows, int ncols, const float *PHIin, int S_in, const float *AA,
                                              const pdeip_dispseg_params *prm, unsigned long long seed, int *S_out, float *PHI_out, int *SEG_out,
                                              float *surf_out)
{
    return disp_segmentation("pdeip_disp_segmentation_sparse", true, Din, nrows, ncols, PHIin, S_in, AA, prm, seed, S_out, PHI_out, SEG_out,
                             surf_out);
}
