// pdeip_ransac.hip -- libpdeip.so: SurfaceEquation, the RANSAC fit of a first- or second-order polynomial surface z = f(x, y).
//
//   [M_out, Err] = SurfaceEquation(A, B, M_in, err_thr, min_set_size, iter)   mex/source/SurfaceEquation.c + library/ransac.c
//                                                                              pdeip_surface_equation(_dev)
//   the fit on the pixels with PHI >= 0 of the segmentation drivers, resident (DispSegmentation.m:329-360)
//                                                                              pdeip_surface_fit_masked_dev
//   the same fit of S level-set planes over one data plane in one chain (region competition's fit stage)
//                                                                              pdeip_surface_fit_masked_batch_dev
//
// All three are one chain (run_chain) on one workspace layout (carve): the rows-given call on GivenRows, the masked calls on
// PixelRows behind the compaction, the single one as the batch of S = 1.
// Kernels: csrc/pdeip_ransac.hpp; the contract: include/pdeip.h.  pdeip_set_mode does not apply.
//
// Build (build.py): hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -c, one object per translation unit.
#include "pdeip_ctx.hpp"
#include "pdeip_ransac.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <type_traits>

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
int rows_per_thread(int rows) { return rows >= RS_BIG_ROWS ? RS_R_BIG : 1; }

// Where segment s finds its part of each array of a call's workspace; `rows`: the rows of a segment at most (the masked forms:
// every pixel), whatever the counts turn out to be.  The last three are the masked forms' (null and 0 otherwise).
struct Ws {
    double *psum;  // [S][tiles][H]
    int *pcnt;     // [S][tiles][H]
    float *models; // [S][H][RS_SLOT]
    float *win;    // [S][RS_SLOT]
    int *idx;      // [S][lda]
    int *blk;      // [S][ldb]
    int *ndata;    // [S]
    int lda, ldb, tiles;
};

// Lays the workspace out on `ws` (w == nullptr: only sizes it), the doubles first; every part starts at a multiple of 4 floats.
// Returns its size in floats.
size_t carve(float *ws, int S, int rows, int H, bool masked, Ws *w)
{
    const int nblk = (rows + RS_BLOCK - 1) / RS_BLOCK;
    const size_t tile_rows = (size_t)RS_BLOCK * rows_per_thread(rows), tiles = ((size_t)rows + tile_rows - 1) / tile_rows;
    const size_t np = (size_t)S * tiles * H, lda = masked ? up4((size_t)rows) : 0, ldb = masked ? up4((size_t)nblk) : 0;
    const size_t oCnt = 2 * up4(np), oModels = oCnt + up4(np), oWin = oModels + (size_t)S * H * RS_SLOT, oIdx = oWin + (size_t)S * RS_SLOT;
    const size_t oBlk = oIdx + (size_t)S * lda, oN = oBlk + (size_t)S * ldb, total = oN + (masked ? up4((size_t)S) : 0);
    if (w != nullptr) {
        w->psum = reinterpret_cast<double *>(ws);
        w->pcnt = reinterpret_cast<int *>(ws + oCnt);
        w->models = ws + oModels;
        w->win = ws + oWin;
        w->idx = masked ? reinterpret_cast<int *>(ws + oIdx) : nullptr;
        w->blk = masked ? reinterpret_cast<int *>(ws + oBlk) : nullptr;
        w->ndata = masked ? reinterpret_cast<int *>(ws + oN) : nullptr;
        w->lda = (int)lda;
        w->ldb = (int)ldb;
        w->tiles = (int)tiles;
    }
    return total;
}

// The workspace in `slot`: WS_RANSAC for the single calls; the batch has WS_RANSAC_BATCH to itself, so a single fit between two
// batch calls (or two replays of a captured one) leaves its buffer alone.
int fetch(int slot, int S, int rows, int H, bool masked, Ws *w)
{
    float *ws = nullptr;
    RC(ws_get(slot, carve(nullptr, S, rows, H, masked, nullptr) * sizeof(float), &ws));
    carve(ws, S, rows, H, masked, w);
    return PDEIP_OK;
}

// What one chain runs on: S segments of `rows` rows at most.
struct Call {
    int S, rows;
    const float *M_in; // [S][ncoef] or null
    float err_thr, min_set_size;
    int it;
    const unsigned *sets; // or null: the draws of segment s come from seed + seed_stride*s
    unsigned long long seed, seed_stride;
    float *M_out;
    int *inliers_out;
    double *errsum_out;
    float *err_out;                      // the rows-given form, or null
    const float *PHI, *D;                // the masked forms: [S] planes, one plane
    int nrows;
    float *dist_out;                     //                   [S] planes or null
    int *ndata_out;                      //                   [S] or null
};

// The chain (count -> scan -> scatter ->) fit -> score -> select (-> errors | dist).  The row count of a segment is c.rows (GivenRows)
// or read on the device from w.ndata (PixelRows).
template <int NC, class Src>
int run_chain(hipStream_t s, const Ws &w, const Src &src, const Call &c)
{
    constexpr bool masked = std::is_same<Src, PixelRows>::value;
    const int S = c.S, H = c.it + 1, R = rows_per_thread(c.rows), ndata_h = masked ? 0 : c.rows;
    const dim3 pix((unsigned)((c.rows + RS_BLOCK - 1) / RS_BLOCK), (unsigned)S); // 256-row blocks x segments
    // hypotheses per score block from all the blocks of the call: with few slots and many segments one block takes a tile's every slot
    int G = (int)std::min<long long>(RS_GMAX, std::max<long long>(1, (long long)H * w.tiles * S / RS_WANT_BLOCKS));
    G = std::max(G, (H + 65534) / 65535);
    const float thr2 = c.err_thr * c.err_thr;
    if constexpr (masked) {
        hipLaunchKernelGGL(k_mask_count, pix, dim3(RS_BLOCK), 0, s, c.PHI, c.rows, w.blk, w.ldb);
        hipLaunchKernelGGL(k_mask_scan, dim3((unsigned)S), dim3(RS_SEL_BLOCK), 0, s, w.blk, w.ldb, (int)pix.x, w.ndata, c.ndata_out);
        hipLaunchKernelGGL(k_mask_scatter, pix, dim3(RS_BLOCK), 0, s, c.PHI, c.rows, w.blk, w.ldb, w.idx, w.lda);
        HIPCHK(hipGetLastError());
        tls.last_launches += 3;
    }
    hipLaunchKernelGGL((k_ransac_fit<NC, Src>), dim3((unsigned)(((long long)S * H + 63) / 64)), dim3(64), 0, s, src, ndata_h, w.ndata, S, c.sets,
                       c.seed, c.seed_stride, H, c.M_in, w.models);
    HIPCHK(hipGetLastError());
    const dim3 grid((unsigned)w.tiles, (unsigned)((H + G - 1) / G), (unsigned)S);
    if (R == 1)
        hipLaunchKernelGGL((k_ransac_score<NC, 1, Src>), grid, dim3(RS_BLOCK), 0, s, src, ndata_h, w.ndata, w.models, H, G, thr2, w.psum, w.pcnt);
    else
        hipLaunchKernelGGL((k_ransac_score<NC, RS_R_BIG, Src>), grid, dim3(RS_BLOCK), 0, s, src, ndata_h, w.ndata, w.models, H, G, thr2, w.psum, w.pcnt);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_ransac_select, dim3((unsigned)S), dim3(RS_SEL_BLOCK), 0, s, w.psum, w.pcnt, H, w.tiles, ndata_h, w.ndata, RS_BLOCK * R,
                       w.models, c.M_in != nullptr ? 1 : 0, c.min_set_size, NC, c.M_out, w.win, c.inliers_out, c.errsum_out);
    HIPCHK(hipGetLastError());
    tls.last_launches += 3;
    if constexpr (masked) {
        if (c.dist_out != nullptr) {
            hipLaunchKernelGGL(k_ransac_dist<NC>, pix, dim3(RS_BLOCK), 0, s, c.D, c.nrows, c.rows, w.win, c.dist_out);
            HIPCHK(hipGetLastError());
            tls.last_launches++;
        }
    } else if (c.err_out != nullptr) {
        hipLaunchKernelGGL(k_ransac_errors<NC>, pix, dim3(RS_BLOCK), 0, s, src, c.rows, w.win, c.err_out);
        HIPCHK(hipGetLastError());
        tls.last_launches++;
    }
    return PDEIP_OK;
}

template <class Src>
int run_order(int ncoef, void *stream, const Ws &w, const Src &src, const Call &c)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    return ncoef == 3 ? run_chain<3, Src>(s, w, src, c) : run_chain<6, Src>(s, w, src, c);
}

// The masked calls: S planes on the workspace in `slot`; the refusals of the batch call alone behind `batch`.
int fit_masked(const char *who, bool batch, int slot, void *stream, const float *PHI, const float *D, int nrows, int ncols, int S, int order,
               const float *M_in, float err_thr, float min_set_size, int iter, const unsigned *sets, unsigned long long seed,
               unsigned long long seed_stride, float *M_out, float *dist_out, int *ndata_out)
{
    NONNULL(who, PHI); NONNULL(who, D); NONNULL(who, M_out);
    if (S < 1 || S > 65535) return set_err(PDEIP_ERR_ARG, "%s: S must lie in 1 .. 65535 (got %d)", who, S);
    if (order != 1 && order != 2) return set_err(PDEIP_ERR_ARG, "%s: order must be 1 or 2 (got %d)", who, order);
    const int ncoef = order == 1 ? 3 : 6;
    RC(check_common(who, ncoef, err_thr, min_set_size, iter, M_in));
    if (nrows < 1 || ncols < 1) return set_err(PDEIP_ERR_ARG, "%s: PHI must not be empty (got %dx%d)", who, nrows, ncols);
    if ((long long)nrows * ncols > 0x7fffffffLL / 8) return set_err(PDEIP_ERR_ARG, "%s: image too large", who);
    const int npix = nrows * ncols, it = iter > 0 ? iter : 0;
    if (batch && carve(nullptr, S, npix, it + 1, true, nullptr) > (size_t)INT_MAX)
        return set_err(PDEIP_ERR_ARG, "%s: the workspace of %d planes of %dx%d with %d hypotheses has more than 2^31-1 elements", who, S, nrows, ncols, it);
    if (batch && dist_out != nullptr && (dist_out == PHI || dist_out == D)) return set_err(PDEIP_ERR_ARG, "%s: dist_out must not alias PHI or D", who);
    tls.last_launches = 0;
    Ws w;
    RC(fetch(slot, S, npix, it + 1, true, &w));
    Call c = {};
    c.S = S; c.rows = npix; c.M_in = M_in; c.err_thr = err_thr; c.min_set_size = min_set_size; c.it = it;
    c.sets = sets; c.seed = seed; c.seed_stride = seed_stride; c.M_out = M_out;
    c.PHI = PHI; c.D = D; c.nrows = nrows; c.dist_out = dist_out; c.ndata_out = ndata_out;
    return run_order(ncoef, stream, w, PixelRows{w.idx, w.lda, D, nrows}, c);
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
    const int it = iter > 0 ? iter : 0;
    Ws w;
    RC(fetch(WS_RANSAC, 1, ndata, it + 1, false, &w));
    Call c = {};
    c.S = 1; c.rows = ndata; c.M_in = M_in; c.err_thr = err_thr; c.min_set_size = min_set_size; c.it = it;
    c.sets = sets; c.seed = seed; c.M_out = M_out; c.inliers_out = inliers_out; c.errsum_out = errsum_out; c.err_out = err_out;
    return run_order(ncoef, stream, w, GivenRows{A, B, ndata}, c);
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
    return fit_masked("pdeip_surface_fit_masked_dev", false, WS_RANSAC, stream, PHI, D, nrows, ncols, 1, order, M_in, err_thr, min_set_size, iter,
                      sets, seed, 0, M_out, dist_out, ndata_out);
}

extern "C" int pdeip_surface_fit_masked_batch_dev(void *stream, const float *PHI, const float *D, int nrows, int ncols, int S, int order,
                                                  const float *M_in, float err_thr, float min_set_size, int iter, unsigned long long seed,
                                                  unsigned long long seed_stride, float *M_out, float *dist_out, int *ndata_out)
{
    return fit_masked("pdeip_surface_fit_masked_batch_dev", true, WS_RANSAC_BATCH, stream, PHI, D, nrows, ncols, S, order, M_in, err_thr,
                      min_set_size, iter, nullptr, seed, seed_stride, M_out, dist_out, ndata_out);
}
