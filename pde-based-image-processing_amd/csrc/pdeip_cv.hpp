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
// launches: k_cv_lines runs the column lanes and the row lanes side by side in one grid (the line solve and that grid:
// pdeip_thomas.hpp), k_cv_combine applies the rules.
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

// One Thomas solve of a line L, x written at the line's own positions (base + k*stride).
__device__ __forceinline__ void cv_line(const float *__restrict__ PHI, const float *__restrict__ D, const float *__restrict__ DH,
                                        const float *__restrict__ G, float *__restrict__ x, float *__restrict__ cp,
                                        float *__restrict__ dp, Line L, float tau, float nu)
{
    auto coef_at = [&](int k) __attribute__((always_inline)) { return cv_coef(PHI, D, DH, G, L.base, L.stride, k, L.n, tau, nu); };
    auto store = [&](int k, float v) __attribute__((always_inline)) { x[L.base + (size_t)k * L.stride] = v; };
    thomas::back_plain(cp, dp, L.sbase, L.sstride, L.n, thomas::forward(coef_at, cp, dp, L.sbase, L.sstride, L.n), store);
}

// Both line kinds in one grid (thomas::lane_of), blockIdx.y = frame.  xc / xr are written in the image layout.
__global__ void __launch_bounds__(BLOCK) k_cv_lines(const float *__restrict__ PHI, const float *__restrict__ D,
                                                    const float *__restrict__ DH, const float *__restrict__ G,
                                                    float *__restrict__ xc, float *__restrict__ xr, float *__restrict__ cpc,
                                                    float *__restrict__ dpc, float *__restrict__ cpr, float *__restrict__ dpr,
                                                    int nrows, int ncols, int row_blocks, float tau, float nu)
{
    const size_t fo = (size_t)blockIdx.y * nrows * ncols;
    const thomas::Lane l = thomas::lane_of(blockIdx.x, row_blocks, nrows, ncols);
    if (l.kind == thomas::ROW) cv_line(PHI, D, DH, G, xr, cpr, dpr, thomas::row_line(fo, l.idx, nrows, ncols), tau, nu);
    else if (l.kind == thomas::COL) cv_line(PHI, D, DH, G, xc, cpc, dpc, thomas::col_line(fo, l.idx, nrows, ncols), tau, nu);
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
