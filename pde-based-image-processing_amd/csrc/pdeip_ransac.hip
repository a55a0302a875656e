// pdeip_ransac.hip -- libpdeip.so: SurfaceEquation, the RANSAC fit of a first- or second-order polynomial surface z = f(x, y).
//
//   [M_out, Err] = SurfaceEquation(A, B, M_in, err_thr, min_set_size, iter)   mex/source/SurfaceEquation.c + library/ransac.c
//                                                                              pdeip_surface_equation(_dev)
//   the fit on the pixels with PHI >= 0 of the segmentation drivers, resident (DispSegmentation.m:329-360)
//                                                                              pdeip_surface_fit_masked_dev
//   the same fit of S level-set planes over one data plane in one chain (region competition's fit stage)
//                                                                              pdeip_surface_fit_masked_batch_dev
//
// Kernels: csrc/pdeip_ransac.hpp, csrc/pdeip_ransac_batch.hpp; the contract: include/pdeip.h.  pdeip_set_mode does not apply.
//
// Build (build.py): hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -c, one object per translation unit.
#include "pdeip_ctx.hpp"
#include "pdeip_ransac.hpp"
#include "pdeip_ransac_batch.hpp"

#include <algorithm>
#include <climits>
#include <cmath>

using namespace pdeip;
using namespace pdeip::ransac;

namespace {

constexpr int RS_R_BIG = 4;         // rows per thread of a score block from RS_BIG_ROWS data rows on, 1 below
constexpr int RS_BIG_ROWS = 32768;
constexpr int RS_WANT_BLOCKS = 2048; // score blocks aimed at (256 CUs, 8 blocks each) when choosing the hypotheses per block

int check_common(const char *who, int ncoef, float err_thr, float min_set_size, int iter, const float *M_in)
{
    if (ncoef != 3 && ncoef != 6)
        return set_err(PDEIP_ERR_ARG, "%s: only 1st and 2nd order polynomials are implemented (ncoef = %d, not 3 or 6)", who, ncoef);
    if (!std::isfinite(err_thr)) return set_err(PDEIP_ERR_ARG, "%s: err_thr must be finite", who);
    if (!std::isfinite(min_set_size)) return set_err(PDEIP_ERR_ARG, "%s: min_set_size must be finite", who);
    if (iter <= 0 && M_in == nullptr) return set_err(PDEIP_ERR_ARG, "%s: no hypotheses (iter = %d) and no given model: nothing to return", who, iter);
    if (iter > (RS_GMAX * 65535) - 1) return set_err(PDEIP_ERR_ARG, "%s: iter = %d is too large", who, iter);
    return PDEIP_OK;
}

size_t up4(size_t n) { return (n + 3) & ~(size_t)3; }

// The chain fit -> score -> select (-> errors) on `max_rows` rows at most; the row count itself is ndata_h or, when ndata_d is
// given, read on the device.  ws: at least ransac_ws_floats(max_rows, H) floats.
struct Chain {
    float *models, *win;
    double *psum;
    int *pcnt;
};
int rows_per_thread(int max_rows) { return max_rows >= RS_BIG_ROWS ? RS_R_BIG : 1; }
size_t chain_tiles(int max_rows) { return ((size_t)max_rows + (size_t)RS_BLOCK * rows_per_thread(max_rows) - 1) / ((size_t)RS_BLOCK * rows_per_thread(max_rows)); }
size_t chain_floats(int max_rows, int H) { return up4((size_t)H * RS_SLOT) + 8 + 2 * chain_tiles(max_rows) * H + up4(chain_tiles(max_rows) * H); }
Chain chain_carve(float *ws, int max_rows, int H)
{
    Chain c;
    const size_t np = chain_tiles(max_rows) * H;
    c.psum = reinterpret_cast<double *>(ws); // first: 8-byte aligned (hipMalloc'd base, offsets in multiples of 4 floats)
    c.pcnt = reinterpret_cast<int *>(ws + 2 * np);
    c.models = ws + 2 * np + up4(np);
    c.win = c.models + up4((size_t)H * RS_SLOT);
    return c;
}

template <int NC>
int run_chain(hipStream_t s, const Chain &c, const float *A, const float *B, int lda, int max_rows, int ndata_h, const int *ndata_d,
              const float *M_in, float err_thr, float min_set_size, int iter, const unsigned *sets, unsigned long long seed,
              float *M_out, float *err_out, int *inliers_out, double *errsum_out)
{
    const int it = iter > 0 ? iter : 0, H = it + 1;
    const int R = rows_per_thread(max_rows);
    const int tiles = (int)chain_tiles(max_rows);
    int G = (int)std::min<long long>(RS_GMAX, std::max<long long>(1, (long long)H * tiles / RS_WANT_BLOCKS));
    G = std::max(G, (H + 65534) / 65535);
    const float thr2 = err_thr * err_thr;
    hipLaunchKernelGGL(k_ransac_fit<NC>, dim3((unsigned)((H + 63) / 64)), dim3(64), 0, s, A, B, lda, ndata_h, ndata_d, sets, seed, it, M_in,
                       c.models);
    HIPCHK(hipGetLastError());
    const dim3 grid((unsigned)tiles, (unsigned)((H + G - 1) / G));
    if (R == 1)
        hipLaunchKernelGGL((k_ransac_score<NC, 1>), grid, dim3(RS_BLOCK), 0, s, A, B, lda, ndata_h, ndata_d, c.models, H, G, thr2, c.psum, c.pcnt);
    else
        hipLaunchKernelGGL((k_ransac_score<NC, RS_R_BIG>), grid, dim3(RS_BLOCK), 0, s, A, B, lda, ndata_h, ndata_d, c.models, H, G, thr2, c.psum, c.pcnt);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_ransac_select, dim3(1), dim3(RS_SEL_BLOCK), 0, s, c.psum, c.pcnt, H, ndata_h, ndata_d, RS_BLOCK * R, c.models,
                       M_in != nullptr ? 1 : 0, min_set_size, NC, M_out, c.win, inliers_out, errsum_out);
    HIPCHK(hipGetLastError());
    tls.last_launches += 3;
    if (err_out != nullptr) {
        hipLaunchKernelGGL(k_ransac_errors<NC>, dim3((unsigned)(((size_t)max_rows + RS_BLOCK - 1) / RS_BLOCK)), dim3(RS_BLOCK), 0, s, A, B, lda,
                           ndata_h, ndata_d, c.win, err_out);
        HIPCHK(hipGetLastError());
        tls.last_launches++;
    }
    return PDEIP_OK;
}

} // namespace

extern "C" int pdeip_surface_equation_dev(void *stream, const float *A, const float *B, int ndata, int ncoef, const float *M_in,
                                          float err_thr, float min_set_size, int iter, const unsigned *sets, unsigned long long seed,
                                          float *M_out, float *err_out, int *inliers_out, double *errsum_out)
{
    const char *who = "pdeip_surface_equation_dev";
    NONNULL(who, A); NONNULL(who, B); NONNULL(who, M_out); NONNULL(who, err_out);
    RC(check_common(who, ncoef, err_thr, min_set_size, iter, M_in));
    if (ndata < 1) return set_err(PDEIP_ERR_ARG, "%s: ndata must be >= 1 (got %d)", who, ndata);
    tls.last_launches = 0;
    const int H = (iter > 0 ? iter : 0) + 1;
    float *ws = nullptr;
    RC(ws_get(WS_RANSAC, chain_floats(ndata, H) * sizeof(float), &ws));
    const Chain c = chain_carve(ws, ndata, H);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (ncoef == 3)
        return run_chain<3>(s, c, A, B, ndata, ndata, ndata, nullptr, M_in, err_thr, min_set_size, iter, sets, seed, M_out, err_out, inliers_out, errsum_out);
    return run_chain<6>(s, c, A, B, ndata, ndata, ndata, nullptr, M_in, err_thr, min_set_size, iter, sets, seed, M_out, err_out, inliers_out, errsum_out);
}

extern "C" int pdeip_surface_equation(const float *A, const float *B, int ndata, int ncoef, const float *M_in, float err_thr,
                                      float min_set_size, int iter, const unsigned *sets, unsigned long long seed, float *M_out,
                                      float *err_out, int *inliers_out, double *errsum_out)
{
    const char *who = "SurfaceEquation";
    NONNULL(who, A); NONNULL(who, B); NONNULL(who, M_out); NONNULL(who, err_out);
    RC(check_common(who, ncoef, err_thr, min_set_size, iter, M_in));
    if (ndata < 1) return set_err(PDEIP_ERR_ARG, "%s: ndata must be >= 1 (got %d)", who, ndata);
    const int it = iter > 0 ? iter : 0, H = it + 1, n = ncoef + 1;
    if (sets != nullptr)
        for (size_t k = 0; k < (size_t)it * n; k++)
            if (sets[k] >= (unsigned)ndata)
                return set_err(PDEIP_ERR_ARG, "%s: sets[%zu] = %u is not a row of the %d data", who, k, sets[k], ndata);
    RC(use_device());
    const size_t nA = up4((size_t)ndata * ncoef), nB = up4((size_t)ndata), nS = sets ? up4((size_t)it * n) : 0, nH = up4((size_t)H);
    float *ar = nullptr;
    RC(ws_get(WS_ARENA, (2 * nH + nA + 2 * nB + nS + nH + 16) * sizeof(float), &ar));
    double *dSum = reinterpret_cast<double *>(ar);
    float *dA = ar + 2 * nH, *dB = dA + nA, *dE = dB + nB, *dMi = dE + nB, *dMo = dMi + 8;
    unsigned *dS = reinterpret_cast<unsigned *>(dMo + 8);
    int *dI = reinterpret_cast<int *>(dMo + 8 + nS);
    HIPCHK(hipMemcpy(dA, A, (size_t)ndata * ncoef * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dB, B, (size_t)ndata * sizeof(float), hipMemcpyHostToDevice));
    if (M_in) HIPCHK(hipMemcpy(dMi, M_in, ncoef * sizeof(float), hipMemcpyHostToDevice));
    if (sets && it > 0) HIPCHK(hipMemcpy(dS, sets, (size_t)it * n * sizeof(unsigned), hipMemcpyHostToDevice));
    RC(pdeip_surface_equation_dev(nullptr, dA, dB, ndata, ncoef, M_in ? dMi : nullptr, err_thr, min_set_size, iter, sets ? dS : nullptr, seed,
                                  dMo, dE, dI, dSum));
    HIPCHK(hipMemcpy(M_out, dMo, ncoef * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(err_out, dE, (size_t)ndata * sizeof(float), hipMemcpyDeviceToHost));
    if (inliers_out) HIPCHK(hipMemcpy(inliers_out, dI, (size_t)H * sizeof(int), hipMemcpyDeviceToHost));
    if (errsum_out) HIPCHK(hipMemcpy(errsum_out, dSum, (size_t)H * sizeof(double), hipMemcpyDeviceToHost));
    return PDEIP_OK;
}

extern "C" int pdeip_surface_fit_masked_dev(void *stream, const float *PHI, const float *D, int nrows, int ncols, int order,
                                            const float *M_in, float err_thr, float min_set_size, int iter, const unsigned *sets,
                                            unsigned long long seed, float *M_out, float *dist_out, int *ndata_out)
{
    const char *who = "pdeip_surface_fit_masked_dev";
    NONNULL(who, PHI); NONNULL(who, D); NONNULL(who, M_out);
    if (order != 1 && order != 2) return set_err(PDEIP_ERR_ARG, "%s: order must be 1 or 2 (got %d)", who, order);
    const int ncoef = order == 1 ? 3 : 6;
    RC(check_common(who, ncoef, err_thr, min_set_size, iter, M_in));
    if (nrows < 1 || ncols < 1) return set_err(PDEIP_ERR_ARG, "%s: PHI must not be empty (got %dx%d)", who, nrows, ncols);
    if ((long long)nrows * ncols > 0x7fffffffLL / 8) return set_err(PDEIP_ERR_ARG, "%s: image too large", who);
    tls.last_launches = 0;
    const int npix = nrows * ncols, H = (iter > 0 ? iter : 0) + 1;
    const int nblk = (npix + RS_BLOCK - 1) / RS_BLOCK;
    const size_t nCh = up4(chain_floats(npix, H)), nA = up4((size_t)npix) * ncoef, nB = up4((size_t)npix);
    float *ws = nullptr;
    RC(ws_get(WS_RANSAC, (nCh + nA + nB + up4((size_t)nblk) + 4) * sizeof(float), &ws));
    const Chain c = chain_carve(ws, npix, H);
    float *cA = ws + nCh, *cB = cA + nA;
    int *blk = reinterpret_cast<int *>(cB + nB), *ndata_d = blk + up4((size_t)nblk);
    const int lda = (int)up4((size_t)npix); // the compacted columns are this far apart, whatever the count turns out to be
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_mask_count, dim3((unsigned)nblk), dim3(RS_BLOCK), 0, s, PHI, npix, blk);
    hipLaunchKernelGGL(k_mask_scan, dim3(1), dim3(RS_SEL_BLOCK), 0, s, blk, nblk, ndata_d, ndata_out);
    if (ncoef == 3) hipLaunchKernelGGL(k_mask_scatter<3>, dim3((unsigned)nblk), dim3(RS_BLOCK), 0, s, PHI, D, nrows, npix, blk, cA, lda, cB);
    else hipLaunchKernelGGL(k_mask_scatter<6>, dim3((unsigned)nblk), dim3(RS_BLOCK), 0, s, PHI, D, nrows, npix, blk, cA, lda, cB);
    HIPCHK(hipGetLastError());
    tls.last_launches = 3;
    if (ncoef == 3)
        RC(run_chain<3>(s, c, cA, cB, lda, npix, 0, ndata_d, M_in, err_thr, min_set_size, iter, sets, seed, M_out, nullptr, nullptr, nullptr));
    else
        RC(run_chain<6>(s, c, cA, cB, lda, npix, 0, ndata_d, M_in, err_thr, min_set_size, iter, sets, seed, M_out, nullptr, nullptr, nullptr));
    if (dist_out != nullptr) {
        if (ncoef == 3) hipLaunchKernelGGL(k_ransac_dist<3>, dim3((unsigned)nblk), dim3(RS_BLOCK), 0, s, D, nrows, npix, c.win, dist_out);
        else hipLaunchKernelGGL(k_ransac_dist<6>, dim3((unsigned)nblk), dim3(RS_BLOCK), 0, s, D, nrows, npix, c.win, dist_out);
        HIPCHK(hipGetLastError());
        tls.last_launches++;
    }
    return PDEIP_OK;
}

// ---- S masks over one data plane in one chain ---------------------------------------------------------------------------------------
namespace {

// The batch call's workspace (WS_RANSAC_BATCH, its own slot: a single fit between two batch calls leaves it alone), the doubles
// first.  Returns its size in floats; every part starts at a multiple of 4 floats.
size_t batch_carve(float *ws, int S, int npix, int H, BatchWs *b)
{
    const int nblk = (npix + RS_BLOCK - 1) / RS_BLOCK;
    const size_t tiles = chain_tiles(npix), np = (size_t)S * tiles * H, lda = up4((size_t)npix), ldb = up4((size_t)nblk);
    const size_t oCnt = 2 * up4(np), oModels = oCnt + up4(np), oWin = oModels + (size_t)S * H * RS_SLOT, oIdx = oWin + (size_t)S * RS_SLOT;
    const size_t oBlk = oIdx + (size_t)S * lda, oN = oBlk + (size_t)S * ldb, total = oN + up4((size_t)S);
    if (b != nullptr) {
        b->psum = reinterpret_cast<double *>(ws);
        b->pcnt = reinterpret_cast<int *>(ws + oCnt);
        b->models = ws + oModels;
        b->win = ws + oWin;
        b->idx = reinterpret_cast<int *>(ws + oIdx);
        b->blk = reinterpret_cast<int *>(ws + oBlk);
        b->ndata = reinterpret_cast<int *>(ws + oN);
        b->lda = (int)lda;
        b->ldb = (int)ldb;
        b->tiles = (int)tiles;
    }
    return total;
}

template <int NC>
int run_batch(hipStream_t s, const BatchWs &w, const float *PHI, const float *D, int nrows, int ncols, int S, const float *M_in, float err_thr,
              float min_set_size, int it, unsigned long long seed, unsigned long long seed_stride, float *M_out, float *dist_out, int *ndata_out)
{
    const int npix = nrows * ncols, H = it + 1, nblk = (npix + RS_BLOCK - 1) / RS_BLOCK;
    const int R = rows_per_thread(npix);
    // hypotheses per score block from all the blocks of the call: with few slots and many segments one block takes a tile's every slot
    int G = (int)std::min<long long>(RS_GMAX, std::max<long long>(1, (long long)H * w.tiles * S / RS_WANT_BLOCKS));
    G = std::max(G, (H + 65534) / 65535);
    const float thr2 = err_thr * err_thr;
    const dim3 pix((unsigned)nblk, (unsigned)S);
    hipLaunchKernelGGL(k_maskb_count, pix, dim3(RS_BLOCK), 0, s, PHI, npix, w.blk, w.ldb);
    hipLaunchKernelGGL(k_maskb_scan, dim3((unsigned)S), dim3(RS_SEL_BLOCK), 0, s, w.blk, w.ldb, nblk, w.ndata, ndata_out);
    hipLaunchKernelGGL(k_maskb_scatter, pix, dim3(RS_BLOCK), 0, s, PHI, npix, w.blk, w.ldb, w.idx, w.lda);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_fitb<NC>, dim3((unsigned)(((long long)S * H + 63) / 64)), dim3(64), 0, s, w.idx, w.lda, D, nrows, w.ndata, S, seed,
                       seed_stride, H, M_in, w.models);
    HIPCHK(hipGetLastError());
    const dim3 grid((unsigned)w.tiles, (unsigned)((H + G - 1) / G), (unsigned)S);
    if (R == 1)
        hipLaunchKernelGGL((k_scoreb<NC, 1>), grid, dim3(RS_BLOCK), 0, s, w.idx, w.lda, D, nrows, w.ndata, w.models, H, G, thr2, w.psum, w.pcnt);
    else
        hipLaunchKernelGGL((k_scoreb<NC, RS_R_BIG>), grid, dim3(RS_BLOCK), 0, s, w.idx, w.lda, D, nrows, w.ndata, w.models, H, G, thr2, w.psum, w.pcnt);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_selectb, dim3((unsigned)S), dim3(RS_SEL_BLOCK), 0, s, w.psum, w.pcnt, H, w.tiles, w.ndata, RS_BLOCK * R, w.models,
                       M_in != nullptr ? 1 : 0, min_set_size, NC, M_out, w.win);
    HIPCHK(hipGetLastError());
    tls.last_launches = 6;
    if (dist_out != nullptr) {
        hipLaunchKernelGGL(k_distb<NC>, pix, dim3(RS_BLOCK), 0, s, D, nrows, npix, w.win, dist_out);
        HIPCHK(hipGetLastError());
        tls.last_launches++;
    }
    return PDEIP_OK;
}

} // namespace

extern "C" int pdeip_surface_fit_masked_batch_dev(void *stream, const float *PHI, const float *D, int nrows, int ncols, int S, int order,
                                                  const float *M_in, float err_thr, float min_set_size, int iter, unsigned long long seed,
                                                  unsigned long long seed_stride, float *M_out, float *dist_out, int *ndata_out)
{
    const char *who = "pdeip_surface_fit_masked_batch_dev";
    NONNULL(who, PHI); NONNULL(who, D); NONNULL(who, M_out);
    if (S < 1 || S > 65535) return set_err(PDEIP_ERR_ARG, "%s: S must lie in 1 .. 65535 (got %d)", who, S);
    if (order != 1 && order != 2) return set_err(PDEIP_ERR_ARG, "%s: order must be 1 or 2 (got %d)", who, order);
    const int ncoef = order == 1 ? 3 : 6;
    RC(check_common(who, ncoef, err_thr, min_set_size, iter, M_in));
    if (nrows < 1 || ncols < 1) return set_err(PDEIP_ERR_ARG, "%s: PHI must not be empty (got %dx%d)", who, nrows, ncols);
    if ((long long)nrows * ncols > 0x7fffffffLL / 8) return set_err(PDEIP_ERR_ARG, "%s: image too large", who);
    const int npix = nrows * ncols, it = iter > 0 ? iter : 0;
    const size_t floats = batch_carve(nullptr, S, npix, it + 1, nullptr);
    if (floats > (size_t)INT_MAX)
        return set_err(PDEIP_ERR_ARG, "%s: the workspace of %d planes of %dx%d with %d hypotheses has more than 2^31-1 elements", who, S, nrows, ncols, it);
    if (dist_out != nullptr && (dist_out == PHI || dist_out == D)) return set_err(PDEIP_ERR_ARG, "%s: dist_out must not alias PHI or D", who);
    tls.last_launches = 0;
    float *ws = nullptr;
    RC(ws_get(WS_RANSAC_BATCH, floats * sizeof(float), &ws));
    BatchWs w;
    batch_carve(ws, S, npix, it + 1, &w);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (ncoef == 3) return run_batch<3>(s, w, PHI, D, nrows, ncols, S, M_in, err_thr, min_set_size, it, seed, seed_stride, M_out, dist_out, ndata_out);
    return run_batch<6>(s, w, PHI, D, nrows, ncols, S, M_in, err_thr, min_set_size, it, seed, seed_stride, M_out, dist_out, ndata_out);
}
