// pdeip_segmentation.hpp -- kernels of the segmentation drivers' inner loop: what regionCompetition() does between the surface fit and
// the Chan-Vese step (matlab/segmentation/DispSegmentation.m:497-646, DispSegmentationSparse.m:511-666).  The contract is in
// include/pdeip.h; tests/segmentation_ref.py restates it.
//
//   k_seg_sizes / k_seg_sizes_final        #{PHI_s >= 0} per segment: ballot + popcount per wave, one partial per (tile, segment),
//                                          one workgroup per segment adds them (integers: exact in any order)
//   k_seg_variance / k_seg_variance_final  n_s and the float64 sum of dist over the counted pixels: the thread's value, the xor
//                                          butterfly over the wave, the four waves in ascending order, one partial per (tile,
//                                          segment); one workgroup adds the partials in ascending tile order (thread s: segment s),
//                                          divides, applies minCOV -- the reduction shape of k_ransac_score / k_ransac_select, the
//                                          wave step shared with them (pdeip_reduce.hpp)
//   k_seg_data                             likelihood, competitor and log-odds per pixel, O(S): two passes over the segments
//   k_seg_label                            the numbered map
//   k_seg_nanfill                          D with its NaNs replaced (the sparse driver's DinNoNaN)
//   k_seeds_init / _exclude / _allowed     generateSeeds(): the initial grid of seeds, plane(~include) = value, the allowed area
// A tile is SG_BLOCK pixels in memory (column-major) order; segments are on blockIdx.y.
#pragma once
#include "pdeip_ctx.hpp"
#include "pdeip_reduce.hpp"

#include <cfloat>

namespace pdeip {
namespace seg {

constexpr int SG_BLOCK = 256; // pixels of a tile = threads of a block (RS_BLOCK of the RANSAC kernels)
constexpr int SG_WAVES = SG_BLOCK / 64;
constexpr int SG_FIN_BLOCK = 256;
constexpr int SG_FIN_AHEAD = 16; // tile partials k_seg_variance_final loads before it adds them

__global__ void __launch_bounds__(SG_BLOCK) k_seg_sizes(const float *__restrict__ PHI, int npix, int tiles, int *__restrict__ part)
{
    __shared__ int s_w[SG_WAVES];
    const int s = blockIdx.y, p = blockIdx.x * SG_BLOCK + threadIdx.x;
    const bool in = p < npix && PHI[(size_t)s * npix + p] >= 0.0f; // a NaN is false, -0.0 is true
    const int c = __popcll(__ballot(in));
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) part[(size_t)s * tiles + blockIdx.x] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

// One workgroup per segment: sizes[s] = the sum of its tile partials.
__global__ void __launch_bounds__(SG_FIN_BLOCK) k_seg_sizes_final(const int *__restrict__ part, int tiles, int *__restrict__ sizes)
{
    __shared__ int s_w[SG_FIN_BLOCK / 64];
    const int s = blockIdx.x, tid = threadIdx.x;
    int c = 0;
    for (int t = tid; t < tiles; t += SG_FIN_BLOCK) c += part[(size_t)s * tiles + t];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((tid & 63) == 0) s_w[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        int tot = 0;
#pragma unroll
        for (int w = 0; w < SG_FIN_BLOCK / 64; w++) tot += s_w[w];
        sizes[s] = tot;
    }
}

// has_cap: only pixels with dist < cap count (a NaN dist fails); without it every mask pixel counts and a NaN propagates.
__global__ void __launch_bounds__(SG_BLOCK) k_seg_variance(const float *__restrict__ PHI, const float *__restrict__ dist, int npix, int tiles,
                                                           int has_cap, double cap, double *__restrict__ psum, int *__restrict__ pcnt)
{
    __shared__ double s_sum[SG_WAVES];
    __shared__ int s_cnt[SG_WAVES];
    const int s = blockIdx.y, tid = threadIdx.x, p = blockIdx.x * SG_BLOCK + tid;
    bool in = false;
    double v = 0.0;
    if (p < npix) {
        const double d = (double)dist[(size_t)s * npix + p];
        in = PHI[(size_t)s * npix + p] >= 0.0f && (!has_cap || d < cap);
        v = in ? d : 0.0;
    }
    const int c = __popcll(__ballot(in));
    const double w = wave_sum(v);
    if ((tid & 63) == 0) {
        s_sum[tid >> 6] = w;
        s_cnt[tid >> 6] = c;
    }
    __syncthreads();
    if (tid == 0) {
        double t = s_sum[0];
        int n = s_cnt[0];
#pragma unroll
        for (int k = 1; k < SG_WAVES; k++) {
            t = t + s_sum[k];
            n += s_cnt[k];
        }
        psum[(size_t)s * tiles + blockIdx.x] = t;
        pcnt[(size_t)s * tiles + blockIdx.x] = n;
    }
}

// One workgroup; thread s adds segment s's partials in ascending tile order.  cov = sum / n, then if (cov < minCOV) cov = minCOV
// (a NaN stays, an empty count gives 0/0 = NaN).
__global__ void __launch_bounds__(SG_FIN_BLOCK) k_seg_variance_final(const double *__restrict__ psum, const int *__restrict__ pcnt, int tiles, int S,
                                                                     double minCOV, double *__restrict__ cov, int *__restrict__ n_out)
{
    for (int s = threadIdx.x; s < S; s += SG_FIN_BLOCK) {
        const double *ps = psum + (size_t)s * tiles;
        const int *pc = pcnt + (size_t)s * tiles;
        double t = 0.0;
        int n = 0, k = 0;
        for (; k + SG_FIN_AHEAD <= tiles; k += SG_FIN_AHEAD) { // the loads of a batch in flight together, the additions still in tile order
            double v[SG_FIN_AHEAD];
            int c[SG_FIN_AHEAD];
#pragma unroll
            for (int j = 0; j < SG_FIN_AHEAD; j++) {
                v[j] = ps[k + j];
                c[j] = pc[k + j];
            }
#pragma unroll
            for (int j = 0; j < SG_FIN_AHEAD; j++) {
                t = t + v[j];
                n += c[j];
            }
        }
        for (; k < tiles; k++) {
            t = t + ps[k];
            n += pc[k];
        }
        double c = __ddiv_rn(t, (double)n);
        if (c < minCOV) c = minCOV;
        cov[s] = c;
        if (n_out) n_out[s] = n;
    }
}

// c = 1/sqrt(2*pi*cov), t = dist/(2*cov), P = c*exp(-t): float64, correctly rounded sqrt and divisions, the device maths library's exp.
__device__ __forceinline__ void likelihood(double cov, float d, double &c, double &t, double &P)
{
    c = __ddiv_rn(1.0, __dsqrt_rn((2.0 * 3.14159265358979323846) * cov));
    t = __ddiv_rn((double)d, 2.0 * cov);
    P = c * exp(-t);
}

enum { STRAT_SURFACE = PDEIP_SEG_SURFACE, STRAT_GREEDY = PDEIP_SEG_GREEDY, STRAT_INVERSE = PDEIP_SEG_INVERSE };

// One thread per pixel, lanes along the contiguous direction; cov[s] is wave-uniform.  Pass 1 keeps the two largest competitor
// values that are not NaN (v_r = P_r, or for `inverse` PHI_r >= 0 ? P_r : 0), the owner of the largest, and any(PHI >= 0).  Pass 2
// forms P_s again (the same operations: the same bits) and takes max_{r != s} as the largest unless s owns it, then the second.
// MATLAB's max: NaNs are ignored, all NaN gives NaN, and (this library) the empty set of S == 1 gives 0.
template <int STRAT>
__global__ void __launch_bounds__(SG_BLOCK) k_seg_data(const float *__restrict__ dist, const float *__restrict__ PHI, const float *__restrict__ DH,
                                                       const double *__restrict__ cov, int npix, int S, float *__restrict__ DATA,
                                                       double *__restrict__ P_out)
{
    const int p = blockIdx.x * SG_BLOCK + threadIdx.x;
    if (p >= npix) return;
    double m1 = 0.0, m2 = 0.0;
    int o1 = -1, nn = 0;
    bool any = false;
    for (int s = 0; s < S; s++) {
        const size_t at = (size_t)s * npix + p;
        double c, t, P;
        likelihood(cov[s], dist[at], c, t, P);
        const bool in = PHI[at] >= 0.0f;
        any = any || in;
        const double v = (STRAT == STRAT_INVERSE && !in) ? 0.0 : P;
        if (v == v) {
            if (nn == 0 || v > m1) {
                m2 = m1;
                m1 = v;
                o1 = s;
            } else if (nn == 1 || v > m2) {
                m2 = v;
            }
            nn = nn < 2 ? nn + 1 : 2;
        }
    }
    const double eps = DBL_EPSILON, qnan = __longlong_as_double(0x7ff8000000000000ll);
    for (int s = 0; s < S; s++) {
        const size_t at = (size_t)s * npix + p;
        double c, t, P;
        likelihood(cov[s], dist[at], c, t, P);
        const bool have = s == o1 ? nn >= 2 : nn >= 1; // a competitor r != s whose value is not NaN exists
        const double oth = s == o1 ? m2 : m1;
        double WC;
        if (STRAT == STRAT_INVERSE) {
            const double Q = -(c * expm1(-t)); // the inverse likelihood c - P without the cancellation
            WC = have ? (Q == Q ? (Q > oth ? Q : oth) : oth) : Q;
        } else {
            WC = S == 1 ? 0.0 : (have ? oth : qnan);
            if (STRAT == STRAT_GREEDY && !any && DH[at] > 0.02f) WC = 0.0;
        }
        DATA[at] = (float)log(__ddiv_rn(P + eps, WC + eps));
        if (P_out) P_out[at] = P;
    }
}

// SEG = sum_s s*[PHI_s > 0] over 1-based s, 0 where two or more segments hold the pixel.
__global__ void __launch_bounds__(SG_BLOCK) k_seg_label(const float *__restrict__ PHI, int npix, int S, int *__restrict__ SEG)
{
    const int p = blockIdx.x * SG_BLOCK + threadIdx.x;
    if (p >= npix) return;
    int sum = 0, cnt = 0;
    for (int s = 0; s < S; s++) {
        const bool in = PHI[(size_t)s * npix + p] > 0.0f;
        sum += in ? s + 1 : 0;
        cnt += in ? 1 : 0;
    }
    SEG[p] = cnt >= 2 ? 0 : sum;
}

__global__ void __launch_bounds__(SG_BLOCK) k_seg_nanfill(const float *__restrict__ D, int npix, float fill, float *__restrict__ out)
{
    const int p = blockIdx.x * SG_BLOCK + threadIdx.x;
    if (p >= npix) return;
    const float d = D[p];
    out[p] = d != d ? fill : d;
}

// ---- generateSeeds(): its per-pixel glue (DispSegmentation.m:238-239, 276-277, 374, 426) ----
// PHIinitial: -1, +1 at the 0-based rows 1, 6, 11, .. <= nrows - 2 and columns 1, 6, .. <= ncols - 2.
__global__ void __launch_bounds__(SG_BLOCK) k_seeds_init(int nrows, int ncols, float *__restrict__ PHI)
{
    const int p = blockIdx.x * SG_BLOCK + threadIdx.x;
    if (p >= nrows * ncols) return;
    const int i = p % nrows, j = p / nrows;
    const bool on = i >= 1 && i <= nrows - 2 && j >= 1 && j <= ncols - 2 && (i - 1) % 5 == 0 && (j - 1) % 5 == 0;
    PHI[p] = on ? 1.0f : -1.0f;
}

// plane(~(AA > thr)) = value; a NaN AA is outside.
__global__ void __launch_bounds__(SG_BLOCK) k_seeds_exclude(const float *__restrict__ AA, int npix, float thr, float value, float *__restrict__ plane)
{
    const int p = blockIdx.x * SG_BLOCK + threadIdx.x;
    if (p >= npix) return;
    if (!(AA[p] > thr)) plane[p] = value;
}

// AA = (PHI < 0) && (AA != 0), as 1 / 0.
__global__ void __launch_bounds__(SG_BLOCK) k_seeds_allowed(const float *__restrict__ PHI, int npix, float *__restrict__ AA)
{
    const int p = blockIdx.x * SG_BLOCK + threadIdx.x;
    if (p >= npix) return;
    AA[p] = (PHI[p] < 0.0f && AA[p] != 0.0f) ? 1.0f : 0.0f;
}

} // namespace seg
} // namespace pdeip
