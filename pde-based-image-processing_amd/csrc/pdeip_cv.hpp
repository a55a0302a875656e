// pdeip_cv.hpp -- the Chan-Vese AOS step (CV_solver_2d -> CV_AOSOMP_4_2d, library/levelsetSolvers.c:103, column pass :189,
// row pass :305, GRADNORM_ZERO_CHECK defined, PMIN/PMAX = -5/+5) and the terms the segmentation drivers build for it.
//
// The gateway hands DH to the library's GradNorm_in slot and GradNorm to its Diff_in slot, so with g = GradNorm, delta = DH the
// coefficients are the AC step's harm() with Diff := g, GN := delta, and the right-hand side is d = PHI + (tau*delta)*D.
// Unlike the AC step, the back-substitution chain always runs on the solved x (a g == 0 pixel only changes what is written),
// so the column solve xc and the row solve xr are independent and the reference's two sequential passes are the elementwise
//   col = (i >= 1 && g == 0) ? clamp(PHI) : clamp(0.0f + xc)
//   out = (j >= 1 && g == 0) ? clamp(PHI) : clamp(col + xr)
// (the first element of a line is never tested; 0.0f + xc because the output array starts as zeros).  So the step is two
// launches: k_cv_lines runs the column lanes and the row lanes side by side in one grid, k_cv_combine applies the rules.
//
// clamp is the reference's pair of ifs, not fminf/fmaxf: a NaN passes through.
#pragma once
#include "pdeip_levelset.hpp"

namespace pdeip {
namespace ls {

__device__ __forceinline__ float cv_clamp(float v)
{
    if (v > 5.0f) v = 5.0f;
    if (v < -5.0f) v = -5.0f;
    return v;
}

// a, b, c, d of element k: aos_coef's diffusivities with (GN, Diff) := (DH, G), the CV right-hand side (:226-247, :342-366)
__device__ __forceinline__ Coef cv_coef(const float *__restrict__ PHI, const float *__restrict__ D, const float *__restrict__ DH,
                                        const float *__restrict__ G, size_t base, size_t stride, int k, int n, float tau, float nu)
{
    Coef r = aos_coef(PHI, D, DH, G, base, stride, k, n, tau, nu);
    const size_t pos = base + (size_t)k * stride;
    r.d = PHI[pos] + (tau * DH[pos]) * D[pos];
    return r;
}

// One Thomas solve of a line: the forward sweep of aos_line (LS_CH elements' coefficients fetched ahead of the chain), then
// x[n-1] = dp[n-1], x[k] = dp[k] - cp[k]*x[k+1] written to x at the line's own positions (base + k*stride).
__device__ __forceinline__ void cv_line(const float *__restrict__ PHI, const float *__restrict__ D, const float *__restrict__ DH,
                                        const float *__restrict__ G, float *__restrict__ x, float *__restrict__ cp,
                                        float *__restrict__ dp, size_t base, size_t stride, size_t sbase, size_t sstride, int n,
                                        float tau, float nu)
{
    Coef c0 = cv_coef(PHI, D, DH, G, base, stride, 0, n, tau, nu);
    float cpv = c0.c / c0.b;
    float dpv = c0.d / c0.b;
    cp[sbase] = cpv;
    dp[sbase] = dpv;
    for (int k0 = 1; k0 <= n - 2; k0 += LS_CH) {
        Coef c[LS_CH];
#pragma unroll
        for (int u = 0; u < LS_CH; ++u) c[u] = cv_coef(PHI, D, DH, G, base, stride, min(k0 + u, n - 2), n, tau, nu);
#pragma unroll
        for (int u = 0; u < LS_CH; ++u) {
            const int k = k0 + u;
            if (k <= n - 2) {
                const float div = 1.0f / (c[u].b - cpv * c[u].a);
                cpv = c[u].c * div;
                dpv = (c[u].d - dpv * c[u].a) * div;
                cp[sbase + (size_t)k * sstride] = cpv;
                dp[sbase + (size_t)k * sstride] = dpv;
            }
        }
    }
    {
        const Coef cl = cv_coef(PHI, D, DH, G, base, stride, n - 1, n, tau, nu);
        dpv = (cl.d - dpv * cl.a) / (cl.b - cpv * cl.a); // the last element divides (:247, :368)
    }
    float x1 = dpv;
    x[base + (size_t)(n - 1) * stride] = x1;
    for (int k0 = n - 2; k0 >= 0; k0 -= LS_CH) {
        float cpk[LS_CH], dpk[LS_CH];
#pragma unroll
        for (int u = 0; u < LS_CH; ++u) {
            const int k = max(k0 - u, 0);
            cpk[u] = cp[sbase + (size_t)k * sstride];
            dpk[u] = dp[sbase + (size_t)k * sstride];
        }
#pragma unroll
        for (int u = 0; u < LS_CH; ++u) {
            const int k = k0 - u;
            if (k >= 0) {
                x1 = dpk[u] - cpk[u] * x1;
                x[base + (size_t)k * stride] = x1;
            }
        }
    }
}

// Both line kinds in one grid, one wave per block.  blockIdx.y = frame; blockIdx.x < row_blocks: row lanes (row i, the longer
// chains at landscape shapes, dispatched first), else column lanes (column j).  Row lanes: cp/dp share the image layout.
// Column lanes: cp/dp transposed (element i of column j at i*ncols + j) so that a wave's scratch traffic is one contiguous run.
// xc / xr are written in the image layout.
__global__ void __launch_bounds__(LS_BLOCK) k_cv_lines(const float *__restrict__ PHI, const float *__restrict__ D,
                                                       const float *__restrict__ DH, const float *__restrict__ G,
                                                       float *__restrict__ xc, float *__restrict__ xr, float *__restrict__ cpc,
                                                       float *__restrict__ dpc, float *__restrict__ cpr, float *__restrict__ dpr,
                                                       int nrows, int ncols, int row_blocks, float tau, float nu)
{
    const size_t fo = (size_t)blockIdx.y * nrows * ncols;
    if ((int)blockIdx.x < row_blocks) {
        const int i = blockIdx.x * LS_BLOCK + threadIdx.x;
        if (i >= nrows) return;
        cv_line(PHI, D, DH, G, xr, cpr, dpr, fo + i, (size_t)nrows, fo + i, (size_t)nrows, ncols, tau, nu);
    } else {
        const int j = ((int)blockIdx.x - row_blocks) * LS_BLOCK + threadIdx.x;
        if (j >= ncols) return;
        cv_line(PHI, D, DH, G, xc, cpc, dpc, fo + (size_t)j * nrows, 1, fo + j, (size_t)ncols, nrows, tau, nu);
    }
}

// The two passes' output rules, pixel (i, j) of frame blockIdx.z.
__global__ void k_cv_combine(const float *__restrict__ PHI, const float *__restrict__ G, const float *__restrict__ xc,
                             const float *__restrict__ xr, float *__restrict__ out, int nrows, int ncols)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = blockIdx.y;
    if (i >= nrows) return;
    const size_t pos = (size_t)blockIdx.z * nrows * ncols + (size_t)j * nrows + i;
    const float phi = PHI[pos];
    const bool zero = G[pos] == 0.0f; // -0.0 counts, NaN does not
    const float col = (i >= 1 && zero) ? cv_clamp(phi) : cv_clamp(0.0f + xc[pos]);
    out[pos] = (j >= 1 && zero) ? cv_clamp(phi) : cv_clamp(col + xr[pos]);
}

// DH = 1/(pi*(c0 + PHI^2/c1)), floored at dh_floor (a NaN floor never applies), and gradPHI = sqrt(dx^2 + dy^2) with the GAC
// drivers' imfilter(PHI, [-1 0 1]*0.5, 'replicate') derivatives (DispSegmentation.m:380-387, DispSegmentationSparse.m:388-396).
__global__ void k_cv_terms(const float *__restrict__ PHI, float *__restrict__ DH, float *__restrict__ G, int nrows, int ncols,
                           float c0, float c1, float dh_floor)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = blockIdx.y;
    if (i >= nrows) return;
    const size_t fo = (size_t)blockIdx.z * nrows * ncols;
    const size_t pos = fo + (size_t)j * nrows + i;
    const Nb q = nb_replicate(PHI + fo, i, j, nrows, ncols);
    float dh = 1.0f / (3.14159265358979323846f * (c0 + (q.p * q.p) / c1));
    if (dh < dh_floor) dh = dh_floor;
    const float dx = dcentral(q.w, q.p, q.e), dy = dcentral(q.n, q.p, q.s);
    DH[pos] = dh;
    G[pos] = sqrtf(dx * dx + dy * dy);
}

} // namespace ls
} // namespace pdeip
