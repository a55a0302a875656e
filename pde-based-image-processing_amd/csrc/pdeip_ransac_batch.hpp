// pdeip_ransac_batch.hpp -- kernels of pdeip_surface_fit_masked_batch_dev: the masked RANSAC fit of S level-set planes over one data
// plane in one chain, the segment on a grid axis of every stage.  The contract is in include/pdeip.h; per segment every stage performs
// the operations of its single-fit counterpart in pdeip_ransac.hpp (whose device functions it calls) on the same inputs, so the
// results carry the same bits.
//
// The compaction keeps pixel indices (idx[s][rank] = p), not data rows: a pixel's row depends on its position only and D is one
// plane for all segments, so fit and score re-form the row with pixel_row<NC>(p % nrows, p / nrows) and read D[p].
//
//   k_maskb_count    grid (256-pixel blocks, S)         block counts of PHI_s >= 0
//   k_maskb_scan     grid (S)                           exclusive scan of a segment's block counts, ndata[s]
//   k_maskb_scatter  grid (256-pixel blocks, S)         idx[s][rank(p)] = p
//   k_fitb           grid (ceil(S*H / 64))              one thread per (segment, slot), packed
//   k_scoreb         grid (tiles, hypothesis groups, S) a block whose first row lies at or past ndata[s] exits at once
//   k_selectb        grid (S)
//   k_distb          grid (256-pixel blocks, S)
#pragma once
#include "pdeip_ransac.hpp"

namespace pdeip {
namespace ransac {

// Where segment s finds its part of each array of the call's workspace.
struct BatchWs {
    double *psum;  // [S][tiles][H]
    int *pcnt;     // [S][tiles][H]
    float *models; // [S][H][RS_SLOT]
    float *win;    // [S][RS_SLOT]
    int *idx;      // [S][lda]
    int *blk;      // [S][ldb]
    int *ndata;    // [S]
    int lda, ldb, tiles;
};

__global__ void __launch_bounds__(RS_BLOCK) k_maskb_count(const float *__restrict__ PHI, int npix, int *__restrict__ blk, int ldb)
{
    const size_t s = blockIdx.y;
    mask_count(PHI + s * npix, npix, blk + s * ldb);
}

__global__ void __launch_bounds__(RS_SEL_BLOCK) k_maskb_scan(int *__restrict__ blk, int ldb, int nblk, int *__restrict__ ndata,
                                                             int *__restrict__ ndata_out)
{
    const size_t s = blockIdx.x;
    mask_scan(blk + s * ldb, nblk, ndata + s, ndata_out ? ndata_out + s : nullptr);
}

__global__ void __launch_bounds__(RS_BLOCK) k_maskb_scatter(const float *__restrict__ PHI, int npix, const int *__restrict__ blk, int ldb,
                                                            int *__restrict__ idx, int lda)
{
    const size_t s = blockIdx.y;
    const int rank = mask_rank(PHI + s * npix, npix, blk + s * ldb);
    if (rank >= 0) idx[s * lda + rank] = blockIdx.x * RS_BLOCK + threadIdx.x;
}

// Thread t of the grid is slot t % H of segment t / H: k_ransac_fit's slot on the segment's ranks, seed and count.
template <int NC>
__global__ void __launch_bounds__(64) k_fitb(const int *__restrict__ idx, int lda, const float *__restrict__ D, int nrows,
                                             const int *__restrict__ ndata_d, int S, unsigned long long seed, unsigned long long seed_stride,
                                             int H, const float *__restrict__ M_in, float *__restrict__ models)
{
    constexpr int N = NC + 1;
    const long long t = (long long)blockIdx.x * 64 + threadIdx.x;
    if (t >= (long long)S * H) return;
    const int seg = (int)(t / H), slot = (int)(t - (long long)seg * H);
    float *out = models + (size_t)t * RS_SLOT;
    if (slot == 0) {
        const float *given = M_in != nullptr ? M_in + (size_t)seg * NC : nullptr;
#pragma unroll
        for (int c = 0; c < 6; c++) out[c] = (given != nullptr && c < NC) ? given[c] : 0.0f;
        out[6] = given != nullptr ? 0.0f : 1.0f;
        out[7] = 0.0f;
        return;
    }
    const unsigned ndata = (unsigned)ndata_d[seg];
    const unsigned long long sd = seed + seed_stride * (unsigned long long)seg, h = (unsigned long long)(slot - 1);
    const int *ranks = idx + (size_t)seg * lda;
    double R[N][NC + 1]; // column NC: the right-hand side
    bool singular = false;
#pragma unroll
    for (int k = 0; k < N; k++) {
        const unsigned r = (unsigned)(((splitmix64(sd + h * N + k) >> 32) * (unsigned long long)ndata) >> 32);
        const bool ok = r < ndata;
        singular = singular || !ok;
        const int p = ok ? ranks[r] : 0;
        float a[NC];
        pixel_row<NC>(p % nrows, p / nrows, a);
#pragma unroll
        for (int c = 0; c < NC; c++) R[k][c] = ok ? (double)a[c] : 0.0;
        R[k][NC] = ok ? (double)D[p] : 0.0;
    }
    fit_solve<NC>(R, singular, out);
}

// k_ransac_score's tiles and reduction per segment; the rows are formed once per block, before the hypotheses.
template <int NC, int R>
__global__ void __launch_bounds__(RS_BLOCK) k_scoreb(const int *__restrict__ idx, int lda, const float *__restrict__ D, int nrows,
                                                     const int *__restrict__ ndata_d, const float *__restrict__ models, int H, int G,
                                                     float thr2, double *__restrict__ psum, int *__restrict__ pcnt)
{
    const size_t seg = blockIdx.z;
    const int ndata = ndata_d[seg];
    const long long row0 = (long long)blockIdx.x * (RS_BLOCK * R);
    if (row0 >= ndata) return; // most blocks of a small segment
    const int tid = threadIdx.x;
    const int h0 = blockIdx.y * G;
    const int ng = min(G, H - h0);
    const int *ranks = idx + seg * lda;
    float a[R][NC], b[R];
    bool ok[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const long long row = row0 + (long long)r * RS_BLOCK + tid;
        ok[r] = row < ndata;
        const int p = ok[r] ? ranks[row] : 0;
        pixel_row<NC>(p % nrows, p / nrows, a[r]);
#pragma unroll
        for (int c = 0; c < NC; c++) a[r][c] = ok[r] ? a[r][c] : 0.0f;
        b[r] = ok[r] ? D[p] : 0.0f;
    }
    const size_t at = (seg * gridDim.x + blockIdx.x) * H + h0;
    score_rows<NC, R>(a, b, ok, models + (seg * H + h0) * RS_SLOT, ng, thr2, psum + at, pcnt + at);
}

__global__ void __launch_bounds__(RS_SEL_BLOCK) k_selectb(const double *__restrict__ psum, const int *__restrict__ pcnt, int H, int tiles,
                                                          const int *__restrict__ ndata_d, int tile_rows, const float *__restrict__ models,
                                                          int has_given, float min_set_size, int ncoef, float *__restrict__ M_out,
                                                          float *__restrict__ win)
{
    const size_t seg = blockIdx.x;
    select_winner(psum + seg * tiles * H, pcnt + seg * tiles * H, H, ndata_d[seg], tile_rows, models + seg * H * RS_SLOT, has_given, min_set_size,
                  ncoef, M_out + seg * ncoef, win + seg * RS_SLOT, nullptr, nullptr);
}

template <int NC>
__global__ void __launch_bounds__(RS_BLOCK) k_distb(const float *__restrict__ D, int nrows, int npix, const float *__restrict__ win,
                                                    float *__restrict__ dist_out)
{
    const int p = blockIdx.x * RS_BLOCK + threadIdx.x;
    if (p >= npix) return;
    const size_t seg = blockIdx.y;
    const float *w = win + seg * RS_SLOT;
    float a[NC], m[NC];
    pixel_row<NC>(p % nrows, p / nrows, a);
#pragma unroll
    for (int c = 0; c < NC; c++) m[c] = w[c];
    dist_out[seg * npix + p] = w[6] != 0.0f ? FLT_MAX : row_error<NC>(a, D[p], m);
}

} // namespace ransac
} // namespace pdeip
