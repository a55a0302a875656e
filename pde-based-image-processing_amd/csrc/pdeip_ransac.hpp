// pdeip_ransac.hpp -- kernels of SurfaceEquation: the RANSAC fit of z = f(x, y), f a first- or second-order polynomial
// (mex/source/SurfaceEquation.c + mex/source/library/ransac.c).  The contract is in include/pdeip.h; tests/ransac_ref.py and
// tests/ransac_batch_ref.py restate it.
//
// One call is a chain on one stream, the segment on a grid axis of every stage (S = 1 for the single calls):
//   k_mask_count    grid (256-pixel blocks, S)         block counts of PHI_s >= 0                       } the masked forms:
//   k_mask_scan     grid (S)                           exclusive scan of a segment's block counts,      } pixels ranked in
//                                                      ndata[s] stays on the device                     } column-major order
//   k_mask_scatter  grid (256-pixel blocks, S)         idx[s][rank(p)] = p                              }
//   k_ransac_fit    grid (ceil(S*H / 64))              one thread per (segment, slot), packed: gather, float64 Householder QR, model slot
//   k_ransac_score  grid (tiles, hypothesis groups, S) inlier count and float64 error sum per (tile, hypothesis), stored, no atomics;
//                                                      a block whose first row lies at or past the segment's count exits at once
//   k_ransac_select grid (S)                           sums the partials in tile order, one thread applies RANSAC()'s rules in
//                                                      hypothesis order
//   k_ransac_errors                                    the winner's error vector (the rows-given form)
//   k_ransac_dist   grid (256-pixel blocks, S)         the error of every pixel (the masked forms)
// Fit and score take their data rows from a row source: GivenRows reads the caller's matrix, PixelRows re-forms the row of a
// ranked pixel ([X Y 1] or [X^2 Y^2 XY X Y 1]) and reads D there -- a pixel's row depends on its position only, so the compaction
// keeps indices, not rows.  The number of data rows may live on the device (the masked forms): see rows_of.
#pragma once
#include "pdeip_ctx.hpp"
#include "pdeip_reduce.hpp"

#include <cfloat>

namespace pdeip {
namespace ransac {

constexpr int RS_BLOCK = 256;  // threads of a score / errors / mask block
constexpr int RS_WAVES = RS_BLOCK / 64;
constexpr int RS_GMAX = 32;    // hypotheses of one score block at most
constexpr int RS_SLOT = 8;     // floats of a model slot: coefficients [0..5], [6] != 0: singular, [7] unused
constexpr int RS_SEL_BLOCK = 1024;
constexpr int RS_SEL_CHUNK = 2048; // hypotheses whose totals k_ransac_select holds in LDS at a time

// The rows of segment s: counted on the device (the masked forms) or known on the host (the rows-given form).
__device__ __forceinline__ int rows_of(int ndata_h, const int *ndata_d, size_t s) { return ndata_d ? ndata_d[s] : ndata_h; }

// The output function of SplitMix64 on the state x (Steele, Lea, Flood 2014): next() of a generator whose state is x.
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x)
{
    unsigned long long z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The error of one data row: t = a0*m0; t = t + a1*m1; ...; d = t - b; e = d*d, in single (the unit is built with -ffp-contract=off).
template <int NC>
__device__ __forceinline__ float row_error(const float (&a)[NC], float b, const float (&m)[NC])
{
    float t = a[0] * m[0];
#pragma unroll
    for (int c = 1; c < NC; c++) t = t + a[c] * m[c];
    const float d = t - b;
    return d * d;
}

// Row of pixel (i, j) (0-based) as the drivers build it: X = j + 1, Y = i + 1, every product formed in double and rounded to single.
template <int NC>
__device__ __forceinline__ void pixel_row(int i, int j, float (&a)[NC])
{
    const double X = (double)(j + 1), Y = (double)(i + 1);
    if (NC == 3) {
        a[0] = (float)X; a[1] = (float)Y; a[2] = 1.0f;
    } else {
        a[0] = (float)(X * X); a[1] = (float)(Y * Y); a[2] = (float)(X * Y); a[NC - 3] = (float)X; a[NC - 2] = (float)Y; a[NC - 1] = 1.0f;
    }
}

// ---- row sources: load(s, r, ok, a, b) is row r of segment s, zeros where !ok (nothing is read then) ------------------------------
// SurfaceEquation's caller-supplied matrix (S = 1): columns lda apart.
struct GivenRows {
    const float *A, *B;
    int lda;
    template <int NC>
    __device__ __forceinline__ void load(size_t, long long r, bool ok, float (&a)[NC], float &b) const
    {
#pragma unroll
        for (int c = 0; c < NC; c++) a[c] = ok ? A[(size_t)c * lda + r] : 0.0f;
        b = ok ? B[r] : 0.0f;
    }
};

// The pixels with PHI_s >= 0 by rank (idx[s*lda + r], k_mask_scatter) over the one data plane D of nrows rows.
struct PixelRows {
    const int *idx;
    int lda;
    const float *D;
    int nrows;
    template <int NC>
    __device__ __forceinline__ void load(size_t s, long long r, bool ok, float (&a)[NC], float &b) const
    {
        const unsigned p = ok ? (unsigned)idx[s * lda + r] : 0u, n = (unsigned)nrows; // unsigned: the cheaper division
        pixel_row<NC>((int)(p % n), (int)(p / n), a);
#pragma unroll
        for (int c = 0; c < NC; c++) a[c] = ok ? a[c] : 0.0f;
        b = ok ? D[p] : 0.0f;
    }
};

// ---- fit: slot 0 is the given model (singular when there is none), slot 1 + h hypothesis h ------------------------------------
// Householder QR in float64 without pivoting on the n = NC + 1 samples, every sum in ascending row (column) index, no contraction:
//   for k = 0..NC-1:  s = sum_{i>=k} R[i][k]^2;  norm = sqrt(s);  norm == 0 -> singular;  alpha = R[k][k] > 0 ? -norm : norm;
//                     v_k = R[k][k] - alpha, v_i = R[i][k] (i > k);  vtv = sum_{i>=k} v_i^2;
//                     for every later column c and then the right-hand side:  f = (2*sum_{i>=k} v_i*c_i) / vtv;  c_i = c_i - f*v_i;
//                     R[k][k] = alpha
//   for k = NC-1..0:  t = b[k];  for j = k+1..NC-1: t = t - R[k][j]*x[j];  x[k] = t / R[k][k]
// An index >= ndata (the device forms cannot refuse it) makes the hypothesis singular; nothing is read through it.
// fit_solve: the solve on the gathered samples R (column NC: the right-hand side), and the model slot it fills.
template <int NC>
__device__ __forceinline__ void fit_solve(double (&R)[NC + 1][NC + 1], bool singular, float *__restrict__ out)
{
    constexpr int N = NC + 1;
#pragma unroll
    for (int k = 0; k < NC; k++) {
        double s = 0.0;
#pragma unroll
        for (int i = k; i < N; i++) s = s + R[i][k] * R[i][k];
        const double norm = __dsqrt_rn(s);
        if (norm == 0.0) singular = true;
        const double alpha = R[k][k] > 0.0 ? -norm : norm;
        double v[N];
        v[k] = R[k][k] - alpha;
#pragma unroll
        for (int i = k + 1; i < N; i++) v[i] = R[i][k];
        double vtv = 0.0;
#pragma unroll
        for (int i = k; i < N; i++) vtv = vtv + v[i] * v[i];
#pragma unroll
        for (int c = k + 1; c <= NC; c++) {
            double dot = 0.0;
#pragma unroll
            for (int i = k; i < N; i++) dot = dot + v[i] * R[i][c];
            const double f = __ddiv_rn(2.0 * dot, vtv);
#pragma unroll
            for (int i = k; i < N; i++) R[i][c] = R[i][c] - f * v[i];
        }
        R[k][k] = alpha;
    }
    double x[NC];
#pragma unroll
    for (int k = NC - 1; k >= 0; k--) {
        double t = R[k][NC];
#pragma unroll
        for (int j = k + 1; j < NC; j++) t = t - R[k][j] * x[j];
        x[k] = __ddiv_rn(t, R[k][k]);
    }
#pragma unroll
    for (int c = 0; c < 6; c++) out[c] = (c < NC && !singular) ? (float)x[c < NC ? c : 0] : 0.0f; // a singular hypothesis has the zero model
    out[6] = singular ? 1.0f : 0.0f;
    out[7] = 0.0f;
}

// Thread t of the grid is slot t % H of segment t / H, on the segment's rows, count, given model and seed (seed + seed_stride*s).
// The order-2 solve holds 7 x 7 doubles and sits just below 128 VGPRs; amdgpu_waves_per_eu(4) keeps the allocator from trading its
// four waves per SIMD for a shorter schedule (order 1 needs 59 and is not affected).
template <int NC, class Src>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4)))
k_ransac_fit(Src src, int ndata_h, const int *__restrict__ ndata_d, int S, const unsigned *__restrict__ sets, unsigned long long seed,
             unsigned long long seed_stride, int H, const float *__restrict__ M_in, float *__restrict__ models)
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
    const unsigned ndata = (unsigned)rows_of(ndata_h, ndata_d, seg);
    const unsigned long long sd = seed + seed_stride * (unsigned long long)seg, h = (unsigned long long)(slot - 1);
    double R[N][NC + 1]; // column NC: the right-hand side
    bool singular = false;
#pragma unroll
    for (int k = 0; k < N; k++) {
        unsigned r;
        if (sets != nullptr) r = sets[h * N + k];
        else r = (unsigned)(((splitmix64(sd + h * N + k) >> 32) * (unsigned long long)ndata) >> 32);
        const bool ok = r < ndata;
        singular = singular || !ok;
        float a[NC], b;
        src.template load<NC>(seg, r, ok, a, b);
#pragma unroll
        for (int c = 0; c < NC; c++) R[k][c] = (double)a[c];
        R[k][NC] = (double)b;
    }
    fit_solve<NC>(R, singular, out);
}

// ---- score: grid (data tiles, hypothesis groups, segments); a tile is RS_BLOCK * R rows, thread t holds rows
// row0 + r*RS_BLOCK + t.
// Per hypothesis: the thread's float64 sum over its inlier rows in ascending r, the xor butterfly over the wave (partners 32, 16,
// .. 1 lanes apart), the four waves in ascending order; the count by ballot + popcount.  One (count, sum) per (tile, hypothesis) is
// stored.  The butterfly runs on eight hypotheses at a time: in its first three steps a lane passes on the partial of the
// hypothesis its partner keeps and keeps the other one, so eight sums cost 4 + 2 + 1 + 3 exchanges instead of 8 * 6.  Every sum
// still goes through the same tree of additions (IEEE addition commutes), so equal models have equal sums wherever they stand.
constexpr int RS_BATCH = 8;

__device__ __forceinline__ double pair_step(double even, double odd, bool upper, int d)
{
    return (upper ? odd : even) + __shfl_xor(upper ? even : odd, d, 64);
}

// The block's part of the scores of `ng` hypotheses on the rows it holds: models, psum and pcnt start at the block's first hypothesis.
template <int NC, int R>
__device__ __forceinline__ void score_rows(const float (&a)[R][NC], const float (&b)[R], const bool (&ok)[R], const float *__restrict__ models,
                                           int ng, float thr2, double *__restrict__ psum, int *__restrict__ pcnt)
{
    __shared__ double s_sum[RS_WAVES][RS_GMAX];
    __shared__ int s_cnt[RS_WAVES][RS_GMAX];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const bool b5 = (lane & 32) != 0, b4 = (lane & 16) != 0, b3 = (lane & 8) != 0;
    const int mine = (b3 ? 4 : 0) + (b4 ? 2 : 0) + (b5 ? 1 : 0); // the hypothesis of a batch whose sum this lane ends up with
    for (int g0 = 0; g0 < ng; g0 += RS_BATCH) {
        double s[RS_BATCH];
        int cnt = 0; // of hypothesis g0 + mine
#pragma unroll
        for (int j = 0; j < RS_BATCH; j++) {
            s[j] = 0.0;
            if (g0 + j < ng) {
                const float *ms = models + (size_t)(g0 + j) * RS_SLOT; // wave-uniform: scalar loads
                float m[NC];
#pragma unroll
                for (int c = 0; c < NC; c++) m[c] = ms[c];
                const bool singular = ms[6] != 0.0f;
                int c1 = 0;
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const float e = singular ? FLT_MAX : row_error<NC>(a[r], b[r], m);
                    const bool in = ok[r] && e <= thr2;
                    c1 += __popcll(__ballot(in));
                    s[j] = s[j] + (in ? (double)e : 0.0);
                }
                cnt = mine == j ? c1 : cnt;
            }
        }
        double t[4], u[2];
#pragma unroll
        for (int j = 0; j < 4; j++) t[j] = pair_step(s[2 * j], s[2 * j + 1], b5, 32); // hypothesis 2j + b5
#pragma unroll
        for (int j = 0; j < 2; j++) u[j] = pair_step(t[2 * j], t[2 * j + 1], b4, 16); // 4j + 2*b4 + b5
        double w = pair_step(u[0], u[1], b3, 8);                                      // 4*b3 + 2*b4 + b5
        w = wave_sum<4>(w);
        if ((lane & 7) == 0 && g0 + mine < ng) {
            s_sum[wave][g0 + mine] = w;
            s_cnt[wave][g0 + mine] = cnt;
        }
    }
    __syncthreads();
    if (tid < ng) {
        double s = s_sum[0][tid];
        int cnt = s_cnt[0][tid];
#pragma unroll
        for (int w = 1; w < RS_WAVES; w++) {
            s = s + s_sum[w][tid];
            cnt += s_cnt[w][tid];
        }
        psum[tid] = s;
        pcnt[tid] = cnt;
    }
}

// The rows are formed once per block, before the hypotheses.
template <int NC, int R, class Src>
__global__ void __launch_bounds__(RS_BLOCK) k_ransac_score(Src src, int ndata_h, const int *__restrict__ ndata_d,
                                                           const float *__restrict__ models, int H, int G, float thr2,
                                                           double *__restrict__ psum, int *__restrict__ pcnt)
{
    const size_t seg = blockIdx.z;
    const int ndata = rows_of(ndata_h, ndata_d, seg);
    const long long row0 = (long long)blockIdx.x * (RS_BLOCK * R);
    if (row0 >= ndata) return; // the masked forms size the grid for every pixel: most blocks of a small segment
    const int tid = threadIdx.x;
    const int h0 = blockIdx.y * G;
    const int ng = min(G, H - h0);
    float a[R][NC], b[R];
    bool ok[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const long long row = row0 + (long long)r * RS_BLOCK + tid;
        ok[r] = row < ndata;
        src.template load<NC>(seg, row, ok[r], a[r], b[r]);
    }
    const size_t at = (seg * gridDim.x + blockIdx.x) * H + h0;
    score_rows<NC, R>(a, b, ok, models + (seg * H + h0) * RS_SLOT, ng, thr2, psum + at, pcnt + at);
}

// ---- select: one workgroup per segment ------------------------------------------------------------------------------------------
// Totals: per hypothesis the tile partials in ascending tile order.  Then thread 0 walks the slots in order with RANSAC()'s rules
// (ransac.c:112-211) and writes the winner's slot to `win` and its coefficients to M_out.
__device__ __forceinline__ void select_winner(const double *__restrict__ psum, const int *__restrict__ pcnt, int H, int ndata, int tile_rows,
                                              const float *__restrict__ models, int has_given, float min_set_size, int ncoef,
                                              float *__restrict__ M_out, float *__restrict__ win, int *__restrict__ inliers_out,
                                              double *__restrict__ errsum_out)
{
    __shared__ double s_sum[RS_SEL_CHUNK];
    __shared__ int s_cnt[RS_SEL_CHUNK];
    const int tiles = ndata / tile_rows + (ndata % tile_rows != 0 ? 1 : 0);
    const int tid = threadIdx.x;
    // abs_min = (unsigned)(min_set_size*(float)ndata + 0.5f); below 1 (negative included) it is 0, from 2^32 on it is 2^32 - 1
    const float amf = min_set_size * (float)ndata + 0.5f;
    const unsigned abs_min = amf < 1.0f ? 0u : (amf >= 4294967296.0f ? 0xffffffffu : (unsigned)amf);
    double best_sum = (double)FLT_MAX;
    int best = -1, inlr = -1, found = 0;
    unsigned best_inlr = 0;
    for (int base = 0; base < H; base += RS_SEL_CHUNK) {
        const int n = min(RS_SEL_CHUNK, H - base);
        for (int k = tid; k < n; k += RS_SEL_BLOCK) {
            double s = 0.0;
            int c = 0;
            for (int t = 0; t < tiles; t++) {
                s = s + psum[(size_t)t * H + base + k];
                c += pcnt[(size_t)t * H + base + k];
            }
            s_sum[k] = s;
            s_cnt[k] = c;
            const bool none = base + k == 0 && !has_given;
            if (inliers_out) inliers_out[base + k] = none ? -1 : c;
            if (errsum_out) errsum_out[base + k] = none ? 0.0 : s;
        }
        __syncthreads();
        if (tid == 0) {
            for (int k = 0; k < n; k++) {
                const int h = base + k;
                const unsigned c = (unsigned)s_cnt[k];
                const double s = s_sum[k];
                if (h == 0) { // the given model seeds the best sum and is licit iff it has enough inliers (:112-144)
                    if (has_given && c >= abs_min) {
                        best_sum = s;
                        best = 0;
                        found = 1;
                    }
                } else if (c >= abs_min && s < best_sum) {
                    found = 1;
                    best = h;
                    best_sum = s;
                } else if (c >= best_inlr && !found) {
                    best_inlr = c;
                    inlr = h;
                }
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        int w = found ? best : inlr;
        if (w < 0) w = 0; // no hypotheses and a given model that is not licit: the given model
        const bool none = ndata == 0 && !has_given; // an empty mask and nothing given: NaN
        for (int c = 0; c < RS_SLOT; c++) {
            const float v = none ? (c < 6 ? __int_as_float(0x7fc00000) : 0.0f) : models[(size_t)w * RS_SLOT + c];
            win[c] = v;
            if (c < ncoef) M_out[c] = v;
        }
    }
}

// `tiles`: the tiles the score grid had, the partials of a segment that far apart.
__global__ void __launch_bounds__(RS_SEL_BLOCK) k_ransac_select(const double *__restrict__ psum, const int *__restrict__ pcnt, int H, int tiles,
                                                                int ndata_h, const int *__restrict__ ndata_d, int tile_rows,
                                                                const float *__restrict__ models, int has_given, float min_set_size,
                                                                int ncoef, float *__restrict__ M_out, float *__restrict__ win,
                                                                int *__restrict__ inliers_out, double *__restrict__ errsum_out)
{
    const size_t seg = blockIdx.x;
    select_winner(psum + seg * tiles * H, pcnt + seg * tiles * H, H, rows_of(ndata_h, ndata_d, seg), tile_rows, models + seg * H * RS_SLOT,
                  has_given, min_set_size, ncoef, M_out + seg * ncoef, win + seg * RS_SLOT, inliers_out ? inliers_out + seg * H : nullptr,
                  errsum_out ? errsum_out + seg * H : nullptr);
}

// ---- the winner's errors on the given rows --------------------------------------------------------------------------------------
template <int NC>
__global__ void __launch_bounds__(RS_BLOCK) k_ransac_errors(GivenRows src, int ndata, const float *__restrict__ win, float *__restrict__ err_out)
{
    const long long row = (long long)blockIdx.x * RS_BLOCK + threadIdx.x;
    if (row >= ndata) return;
    float a[NC], b, m[NC];
    src.load<NC>(0, row, true, a, b);
#pragma unroll
    for (int c = 0; c < NC; c++) m[c] = win[c];
    err_out[row] = win[6] != 0.0f ? FLT_MAX : row_error<NC>(a, b, m);
}

// ---- the masked forms: S level-set planes (npix apart) over one data plane --------------------------------------------------------
// Pixels in memory (column-major) order; PHI >= 0 is false for a NaN.  One block ranks RS_BLOCK pixels.  Segment s has its block
// counts at blk + s*ldb and its ranked pixels at idx + s*lda.
__device__ __forceinline__ void mask_count(const float *__restrict__ PHI, int npix, int *__restrict__ blk_cnt)
{
    __shared__ int s_w[RS_WAVES];
    const int p = blockIdx.x * RS_BLOCK + threadIdx.x;
    const bool in = p < npix && PHI[p] >= 0.0f;
    const int c = __popcll(__ballot(in));
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

__global__ void __launch_bounds__(RS_BLOCK) k_mask_count(const float *__restrict__ PHI, int npix, int *__restrict__ blk, int ldb)
{
    const size_t s = blockIdx.y;
    mask_count(PHI + s * npix, npix, blk + s * ldb);
}

// Exclusive prefix sum of the block counts, in place, by one workgroup; the total goes to ndata[0] and ndata_out[0].
__device__ __forceinline__ void mask_scan(int *__restrict__ blk, int nblk, int *__restrict__ ndata, int *__restrict__ ndata_out)
{
    __shared__ int s[RS_SEL_BLOCK];
    __shared__ int s_carry;
    const int tid = threadIdx.x;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (int base = 0; base < nblk; base += RS_SEL_BLOCK) {
        const int k = base + tid;
        const int v = k < nblk ? blk[k] : 0;
        s[tid] = v;
        __syncthreads();
        for (int d = 1; d < RS_SEL_BLOCK; d <<= 1) {
            const int add = tid >= d ? s[tid - d] : 0;
            __syncthreads();
            s[tid] += add;
            __syncthreads();
        }
        const int carry = s_carry;
        if (k < nblk) blk[k] = carry + s[tid] - v;
        __syncthreads();
        if (tid == RS_SEL_BLOCK - 1) s_carry = carry + s[tid];
        __syncthreads();
    }
    if (tid == 0) {
        ndata[0] = s_carry;
        if (ndata_out) ndata_out[0] = s_carry;
    }
}

__global__ void __launch_bounds__(RS_SEL_BLOCK) k_mask_scan(int *__restrict__ blk, int ldb, int nblk, int *__restrict__ ndata,
                                                            int *__restrict__ ndata_out)
{
    const size_t s = blockIdx.x;
    mask_scan(blk + s * ldb, nblk, ndata + s, ndata_out ? ndata_out + s : nullptr);
}

// The rank of pixel p = blockIdx.x * RS_BLOCK + threadIdx.x among the pixels with PHI >= 0, or -1 when it is not one of them.
__device__ __forceinline__ int mask_rank(const float *__restrict__ PHI, int npix, const int *__restrict__ blk_off)
{
    __shared__ int s_w[RS_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = blockIdx.x * RS_BLOCK + tid;
    const bool in = p < npix && PHI[p] >= 0.0f;
    const unsigned long long bal = __ballot(in);
    if (lane == 0) s_w[wave] = __popcll(bal);
    __syncthreads();
    if (!in) return -1;
    int rank = blk_off[blockIdx.x] + __popcll(bal & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; w++) rank += s_w[w];
    return rank;
}

__global__ void __launch_bounds__(RS_BLOCK) k_mask_scatter(const float *__restrict__ PHI, int npix, const int *__restrict__ blk, int ldb,
                                                           int *__restrict__ idx, int lda)
{
    const size_t s = blockIdx.y;
    const int rank = mask_rank(PHI + s * npix, npix, blk + s * ldb);
    if (rank >= 0) idx[s * lda + rank] = blockIdx.x * RS_BLOCK + threadIdx.x;
}

// dist_out(s, p) = the error formula on the row of pixel p against D(p) with segment s's winner, for every pixel.
template <int NC>
__global__ void __launch_bounds__(RS_BLOCK) k_ransac_dist(const float *__restrict__ D, int nrows, int npix, const float *__restrict__ win,
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
