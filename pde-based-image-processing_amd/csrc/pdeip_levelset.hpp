// pdeip_levelset.hpp -- the level-set kernels: one AOS step of the geodesic active contour (AC_AOS_4_2d,
// library/levelsetSolvers.c:145-181) and the re-initialisation step of reinit() (:969-1118).
//
// AOS.  Every line (column or row of one frame) is one tridiagonal Thomas solve, independent of every other line: one lane
// per line, forward sweep, scratch layout and line geometry from pdeip_thomas.hpp; the back-substitution is this step's own.
// The reference's 2048-element line limit (MAX_BUF_SIZE) does not apply.
//
// Both passes write   out = x + carry   where `carry` is 0 for the column pass (the output array starts as zeros,
// :751-768) and the column result for the row pass (:853-870).  The passes treat Diff == 0 differently, both reproduced:
//   column pass: the pixel's x is PHI_in (and it feeds the next back-substitution step as such);
//   row pass:    the pixel keeps its column value as x (and feeds the chain with it), its carry becomes 0, and the NEXT pixel
//                along the row is overwritten with PHI_in[next] + its carry.
// The last element of a line is never tested.  -ffp-contract=off (build.py) keeps every product and sum separate.
//
// Re-initialisation.  One launch per step, cross-shaped radius-1 neighbourhood of phi, separate output buffer.  The sign
// function is this library's contract: S = PHI * (1/sqrtf(PHI^2 + sqrtf((PHIx^2 + PHIy^2) + FLT_EPSILON)))
// -- the SSE path's operation order with a correctly rounded reciprocal square root instead of rsqrtps.
#pragma once
#include "pdeip_thomas.hpp"

namespace pdeip {
namespace ls {

using thomas::BLOCK;
using thomas::CH;
using thomas::Coef;
using thomas::Line;

// Harmonic diffusivity between `pos` and its neighbour `q` (:705-706): a non-positive or NaN sum gives 0.
__device__ __forceinline__ float harm(const float *__restrict__ Diff, const float *__restrict__ GN, size_t pos, size_t q, float tau)
{
    const float t = Diff[pos] + Diff[q];
    return (t > 0.0f) ? ((2.0f * tau) * GN[pos]) / t : 0.0f;
}

// a, b, c, d of element k of a line of length n whose element k sits at base + k*stride (:702-742, :809-848).
__device__ __forceinline__ Coef aos_coef(const float *__restrict__ PHI, const float *__restrict__ D, const float *__restrict__ GN,
                                         const float *__restrict__ Diff, size_t base, size_t stride, int k, int n, float tau, float nu)
{
    const size_t pos = base + (size_t)k * stride;
    Coef r;
    if (k == 0) {
        const float dn = harm(Diff, GN, pos, pos + stride, tau);
        r.a = 0.0f;
        r.b = 2.0f + nu * dn;
        r.c = (-nu) * dn;
    } else if (k == n - 1) {
        const float dpv = harm(Diff, GN, pos, pos - stride, tau);
        r.a = (-nu) * dpv;
        r.b = 2.0f + nu * dpv;
        r.c = 0.0f;
    } else {
        const float dn = harm(Diff, GN, pos, pos + stride, tau);
        const float dpv = harm(Diff, GN, pos, pos - stride, tau);
        r.a = (-nu) * dpv;
        r.b = 2.0f + nu * (dn + dpv);
        r.c = (-nu) * dn;
    }
    r.d = PHI[pos] + tau * D[pos];
    return r;
}

// One Thomas solve of a line L: thomas::forward (:700-742), then the AOS back-substitution.  ROW selects the row pass's
// Diff == 0 rule and its carry (the column values already in `out`); the column pass has carry 0.
template <bool ROW>
__device__ __forceinline__ void aos_line(const float *__restrict__ PHI, const float *__restrict__ D, const float *__restrict__ GN,
                                         const float *__restrict__ Diff, const float *__restrict__ col, float *__restrict__ out,
                                         float *__restrict__ cp, float *__restrict__ dp, Line L, float tau, float nu)
{
    const size_t base = L.base, stride = L.stride, sbase = L.sbase, sstride = L.sstride;
    const int n = L.n;
    auto coef_at = [&](int k) __attribute__((always_inline)) { return aos_coef(PHI, D, GN, Diff, base, stride, k, n, tau, nu); };
    // ---- back-substitution (:737-768 / :850-876) ----
    // x1/t1: x and carry of element k+1 (the carry of the last element is its column value; it is never tested)
    float x1 = thomas::forward(coef_at, cp, dp, sbase, sstride, n);
    float t1 = ROW ? col[base + (size_t)(n - 1) * stride] : 0.0f;
    for (int k0 = n - 2; k0 >= 0; k0 -= CH) {
        float cpk[CH], dpk[CH], dfk[CH], phk[CH], clk[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int k = max(k0 - u, 0);
            const size_t pos = base + (size_t)k * stride;
            cpk[u] = cp[sbase + (size_t)k * sstride];
            dpk[u] = dp[sbase + (size_t)k * sstride];
            dfk[u] = Diff[pos];
            phk[u] = ROW ? PHI[pos + stride] : PHI[pos];
            clk[u] = ROW ? col[pos] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int k = k0 - u;
            if (k >= 0) {
                const size_t pos = base + (size_t)k * stride;
                const bool zero = dfk[u] == 0.0f;
                float x, t;
                if (ROW) {
                    x = zero ? clk[u] : dpk[u] - cpk[u] * x1;
                    t = zero ? 0.0f : clk[u];
                    out[pos + stride] = (zero ? phk[u] : x1) + t1; // element k+1 is final once k has used it
                } else {
                    x = zero ? phk[u] : dpk[u] - cpk[u] * x1;
                    t = 0.0f;
                    out[pos + stride] = x1 + t1;
                }
                x1 = x;
                t1 = t;
            }
        }
    }
    out[base] = x1 + t1;
}

// Column pass: lane = column j of frame blockIdx.y (thomas::col_line).
__global__ void __launch_bounds__(BLOCK) k_aos_col(const float *__restrict__ PHI, const float *__restrict__ D,
                                                   const float *__restrict__ GN, const float *__restrict__ Diff,
                                                   float *__restrict__ out, float *__restrict__ cp, float *__restrict__ dp,
                                                   int nrows, int ncols, float tau, float nu)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ncols) return;
    const size_t fo = (size_t)blockIdx.y * nrows * ncols;
    aos_line<false>(PHI, D, GN, Diff, nullptr, out, cp, dp, thomas::col_line(fo, j, nrows, ncols), tau, nu);
}

// Row pass: lane = row i of frame blockIdx.y (thomas::row_line); a launch of its own because it reads the column pass.  `col`
// is the column pass's output (read), `out` the sum (written); they may not alias across lanes, and each lane only touches its
// own row of both.
__global__ void __launch_bounds__(BLOCK) k_aos_row(const float *__restrict__ PHI, const float *__restrict__ D,
                                                   const float *__restrict__ GN, const float *__restrict__ Diff,
                                                   const float *__restrict__ col, float *__restrict__ out,
                                                   float *__restrict__ cp, float *__restrict__ dp, int nrows, int ncols,
                                                   float tau, float nu)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nrows) return;
    const size_t fo = (size_t)blockIdx.y * nrows * ncols;
    aos_line<true>(PHI, D, GN, Diff, col, out, cp, dp, thomas::row_line(fo, i, nrows, ncols), tau, nu);
}

__device__ __forceinline__ float maxP2(float A) { return (A > 0.0f) ? (A * A) : 0.0f; } // :41-43
__device__ __forceinline__ float minP2(float A) { return (A < 0.0f) ? (A * A) : 0.0f; }
__device__ __forceinline__ float cmax(float A, float B) { return (A > B) ? A : B; }

// One re-initialisation step phi -> out (:1079-1101), pixel (i, j) of frame blockIdx.z.
__global__ void k_reinit_step(const float *__restrict__ phi, float *__restrict__ out, int nrows, int ncols)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = blockIdx.y;
    if (i >= nrows) return;
    const size_t fo = (size_t)blockIdx.z * nrows * ncols;
    const float *P = phi + fo;
    const size_t pos = (size_t)j * nrows + i;
    const float p = P[pos];
    const float pW = j > 0 ? P[pos - nrows] : p, pE = j < ncols - 1 ? P[pos + nrows] : p;
    const float pN = i > 0 ? P[pos - 1] : p, pS = i < nrows - 1 ? P[pos + 1] : p;
    // HorizontalConv / VerticalConv with {-0.5, 0.5}: central, one-sided at the borders (:882-966)
    const float PHIx = pW * -0.5f + pE * 0.5f;
    const float PHIy = pN * -0.5f + pS * 0.5f;
    // blurred sign function, SSE operation order (:1217-1239), correctly rounded (the contract)
    float g = PHIx * PHIx;
    g = g + PHIy * PHIy;
    g = g + 1.1920928955078125e-07f; // FLT_EPSILON
    g = sqrtf(g);
    const float S = p * (1.0f / sqrtf(g + p * p));
    // Godunov upwind squares, Rouy-Tourin (:1311-1392); a one-sided border difference is 0
    const float xfd = j < ncols - 1 ? pE - p : 0.0f, xbd = j > 0 ? p - pW : 0.0f;
    const float yfd = i < nrows - 1 ? pS - p : 0.0f, ybd = i > 0 ? p - pN : 0.0f;
    float X2, Y2;
    if (S > 0.0f) {
        X2 = cmax(maxP2(xbd), minP2(xfd));
        Y2 = cmax(maxP2(ybd), minP2(yfd));
    } else {
        X2 = cmax(minP2(xbd), maxP2(xfd));
        Y2 = cmax(minP2(ybd), maxP2(yfd));
    }
    // SSE update (:1081-1089): phi + 0.25*(S - sqrt(X2+Y2)*S)
    const float r = sqrtf(X2 + Y2) * S;
    out[fo + pos] = 0.25f * (S - r) + p;
}


// ---- the GAC drivers (matlab/active_contour/GAC_v10a.m:35-121, GAC_v10b.m) ------------------------------------------------
// imfilter(P, m, 'replicate') with a 3-tap mask m along one axis, as pyramid.py defines imfilter: the taps' products summed
// in double in mask order from 0, rounded to single once.  pm, p0, pp: the previous, centre and next sample (replicated).
__device__ __forceinline__ float filt3(float pm, float p0, float pp, double m0, double m1, double m2)
{
    double acc = 0.0;
    acc += m0 * (double)pm;
    acc += m1 * (double)p0;
    acc += m2 * (double)pp;
    return (float)acc;
}
__device__ __forceinline__ float dcentral(float pm, float p0, float pp) { return filt3(pm, p0, pp, -0.5, 0.0, 0.5); } // [-1 0 1]*0.5
__device__ __forceinline__ float pos0(float x) { return x > 0.0f ? x : 0.0f; } // max(x, 0): NaN gives 0 (MATLAB ignores NaN)
__device__ __forceinline__ float neg0(float x) { return x < 0.0f ? x : 0.0f; } // min(x, 0)
// max over channels (max(., [], 3)): NaN ignored, the first of equal values kept
__device__ __forceinline__ float nanmax(float m, float v) { return (v > m || m != m) ? v : m; }

struct Nb {
    float p, n, s, w, e; // centre and its replicated neighbours (north = row - 1, west = column - 1)
};
__device__ __forceinline__ Nb nb_replicate(const float *P, int i, int j, int nrows, int ncols)
{
    const size_t pos = (size_t)j * nrows + i;
    Nb r;
    r.p = P[pos];
    r.n = i > 0 ? P[pos - 1] : r.p;
    r.s = i < nrows - 1 ? P[pos + 1] : r.p;
    r.w = j > 0 ? P[pos - nrows] : r.p;
    r.e = j < ncols - 1 ? P[pos + nrows] : r.p;
    return r;
}

// Igrad = max_c(Idx)^2 + max_c(Idy)^2 of the smoothed channels I [C planes] (:59-69)
__global__ void k_gac_igrad(const float *__restrict__ I, float *__restrict__ Igrad, int nrows, int ncols, int C)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
    if (i >= nrows) return;
    const size_t n = (size_t)nrows * ncols;
    float mx = 0.0f, my = 0.0f;
    for (int c = 0; c < C; c++) {
        const Nb q = nb_replicate(I + c * n, i, j, nrows, ncols);
        const float dx = dcentral(q.w, q.p, q.e), dy = dcentral(q.n, q.p, q.s);
        mx = c == 0 ? dx : nanmax(mx, dx);
        my = c == 0 ? dy : nanmax(my, dy);
    }
    Igrad[(size_t)j * nrows + i] = mx * mx + my * my;
}

// ---- lambda = sort(Igrad(:))(k), k = round(0.7*N) (1-based), by four 8-bit radix passes over an order-preserving key
struct Select {
    unsigned prefix, k;      // key bits chosen so far (above the current digit), rank still to find inside them (1-based)
    unsigned hist[256];
};
__device__ __forceinline__ unsigned sel_key(float x)
{
    const unsigned b = __float_as_uint(x);
    if (x != x) return 0xffffffffu;                // MATLAB's sort puts NaN last
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float sel_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__global__ void k_sel_init(Select *st, unsigned k)
{
    st->hist[threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        st->prefix = 0;
        st->k = k;
    }
}
// histogram of digit `shift` over the keys whose higher digits equal st->prefix
__global__ void __launch_bounds__(256) k_sel_hist(Select *st, const float *__restrict__ x, size_t n, int shift)
{
    __shared__ unsigned h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const unsigned prefix = st->prefix;
    const unsigned hi = shift == 24 ? 0u : (0xffffffffu << (shift + 8));
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
        const unsigned key = sel_key(x[p]);
        if ((key & hi) == prefix) atomicAdd(&h[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&st->hist[threadIdx.x], h[threadIdx.x]);
}
// picks the digit that holds rank k, clears the histogram; after the last digit writes the selected value to *lambda
__global__ void k_sel_pick(Select *st, int shift, float *lambda)
{
    if (threadIdx.x != 0) return;
    unsigned k = st->k, b = 0;
    for (; b < 255u; b++) {
        const unsigned h = st->hist[b];
        if (k <= h) break;
        k -= h;
    }
    st->k = k;
    st->prefix |= b << shift;
    for (int t = 0; t < 256; t++) st->hist[t] = 0;
    if (shift == 0) *lambda = sel_unkey(st->prefix);
}

// g = 1./(1 + Igrad./lambda) (:70-75); lambda: the selected value (device) or the caller's (lam_dev == nullptr), which is then
// also written to *lam_out
__global__ void k_gac_g(const float *__restrict__ Igrad, float *__restrict__ g, size_t n, const float *lam_dev, float lam, float *lam_out)
{
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const float l = lam_dev ? *lam_dev : lam;
    if (p == 0 && lam_dev == nullptr) *lam_out = l;
    const float t = Igrad[p] / l;
    g[p] = 1.0f / (1.0f + t);
}
// gdx, gdy = imfilter(g, [-1 0 1]*0.5 (and its transpose), 'replicate') (GAC_v10b.m:73-74)
__global__ void k_gac_gd(const float *__restrict__ g, float *__restrict__ gdx, float *__restrict__ gdy, int nrows, int ncols)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
    if (i >= nrows) return;
    const Nb q = nb_replicate(g, i, j, nrows, ncols);
    gdx[(size_t)j * nrows + i] = dcentral(q.w, q.p, q.e);
    gdy[(size_t)j * nrows + i] = dcentral(q.n, q.p, q.s);
}

// One iteration's AC_solver_2d inputs (GAC_v10a.m:82-107, GAC_v10b.m:82-100): DATA, gradPHI, Diff.
// MODEL 0 (a): DATA = c*g.*gradPHIUW with the upwind branch on c <= 0.  MODEL 1 (b): the convection term with circshift,
// which wraps around at the borders.
template <int MODEL>
__global__ void k_gac_terms(const float *__restrict__ PHI, const float *__restrict__ g, const float *__restrict__ gdx,
                            const float *__restrict__ gdy, float c, int c_le0, float *__restrict__ DATA, float *__restrict__ gradPHI,
                            float *__restrict__ Diff, int nrows, int ncols)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
    if (i >= nrows) return;
    const size_t pos = (size_t)j * nrows + i;
    const Nb q = nb_replicate(PHI, i, j, nrows, ncols);
    const float PHIdx = dcentral(q.w, q.p, q.e), PHIdy = dcentral(q.n, q.p, q.s);
    float data;
    if (MODEL == 0) {
        const float xfd = filt3(q.w, q.p, q.e, 0.0, -1.0, 1.0), xbd = filt3(q.w, q.p, q.e, -1.0, 1.0, 0.0); // [0 -1 1], [-1 1 0]
        const float yfd = filt3(q.n, q.p, q.s, 0.0, -1.0, 1.0), ybd = filt3(q.n, q.p, q.s, -1.0, 1.0, 0.0);
        float a, b, e, f;
        if (c_le0) { // param.c <= 0, decided on the double
            a = pos0(xbd); b = neg0(xfd); e = pos0(ybd); f = neg0(yfd);
        } else {
            a = neg0(xbd); b = pos0(xfd); e = neg0(ybd); f = pos0(yfd);
        }
        const float uw = sqrtf(((a * a + b * b) + e * e) + f * f);
        data = (c * g[pos]) * uw;
    } else {
        // circshift(P,[0 -1]) -> column j+1, [0 1] -> j-1, [-1 0] -> row i+1, [1 0] -> i-1, all modulo the size
        const float pe = PHI[(size_t)(j + 1 < ncols ? j + 1 : 0) * nrows + i], pw = PHI[(size_t)(j > 0 ? j - 1 : ncols - 1) * nrows + i];
        const float ps = PHI[(size_t)j * nrows + (i + 1 < nrows ? i + 1 : 0)], pn = PHI[(size_t)j * nrows + (i > 0 ? i - 1 : nrows - 1)];
        const float gx = gdx[pos], gy = gdy[pos];
        data = ((pos0(gx) * (pe - q.p) + neg0(gx) * (q.p - pw)) + pos0(gy) * (ps - q.p)) + neg0(gy) * (q.p - pn);
    }
    const float gp = sqrtf((PHIdx * PHIdx + PHIdy * PHIdy) + 2.220446049250313e-16f); // + eps
    DATA[pos] = data;
    gradPHI[pos] = gp;
    Diff[pos] = gp / g[pos];
}

} // namespace ls
} // namespace pdeip
