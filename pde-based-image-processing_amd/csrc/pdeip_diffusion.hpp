// pdeip_diffusion.hpp -- the nonlinear (lagged-diffusivity) diffusion filter matlab/diffusion/Diffusion4_v10.m: the line solves
// of one outer iteration and the combine that ends it.  The weights are the DdiffWeights kernel (k_diffweights6,
// csrc/pdeip_pointwise.hpp) with eps = 0.00001f and the channels as its frames, in its <true> form: the maximum over the channels
// omits a NaN of any channel, as the .m's max(w, [], 3).
//
// One outer iteration (Diffusion4_v10.m:44-62), every channel k of Iout solved independently with the iteration's weights:
//   ver = TDMA(-alpha*wN, 2 + alpha*(wN + wS), -alpha*wS, Iout(:,:,k))     along every column
//   hor = TDMA(-alpha*wW, 2 + alpha*(wW + wE), -alpha*wE, Iout(:,:,k))     along every row
//   Iout(:,:,k) = ver + hor
// alpha is the single the double parameter rounds to.  TDMA (:70-92) is the Thomas solve of the level-set lines (cv_line):
// c/b and d/b at the first element, 1/(b - a*c') and two multiplies in the middle, a true division at the last element,
// x = d - c*x' back.  Both solves read the iteration's input, so the column lanes and the row lanes run side by side in one
// launch (k_diff4_lines, the grid of k_cv_lines) and a second, elementwise launch (k_diff4_combine) adds them.
// -ffp-contract=off (build.py) keeps every product and sum separate.
#pragma once
#include <hip/hip_runtime.h>

namespace pdeip {
namespace diff {

constexpr int D4_CH = 8;     // elements whose coefficients are fetched ahead of the chain (the level-set lines' LS_CH)
constexpr int D4_BLOCK = 64; // one wave per block, as the level-set lines

struct D4Coef {
    float a, b, c, d;
};

// a, b, c, d of the element at weight-plane position wpos: wP is the weight towards the previous element of the line (wN for a
// column, wW for a row), wQ the one towards the next (wS, wE); d is the channel's value there.  na = -alpha, al = alpha.
__device__ __forceinline__ D4Coef d4_coef(const float *__restrict__ wP, const float *__restrict__ wQ, const float *__restrict__ I,
                                          size_t wpos, size_t fo, float na, float al)
{
    const float p = wP[wpos], q = wQ[wpos];
    D4Coef r;
    r.a = na * p;
    r.b = 2.0f + al * (p + q);
    r.c = na * q;
    r.d = I[fo + wpos];
    return r;
}

// One Thomas solve of a line of n >= 2 elements whose element k sits at base + k*stride of a weight plane (fo + that in the
// channel): the forward sweep with D4_CH elements' coefficients fetched ahead of the chain into cp/dp at sbase + k*sstride,
// then x[n-1] = dp[n-1], x[k] = dp[k] - cp[k]*x[k+1] written to x at fo + base + k*stride.
__device__ __forceinline__ void d4_line(const float *__restrict__ wP, const float *__restrict__ wQ, const float *__restrict__ I,
                                        float *__restrict__ x, float *__restrict__ cp, float *__restrict__ dp, size_t fo, size_t base,
                                        size_t stride, size_t sbase, size_t sstride, int n, float na, float al)
{
    const D4Coef c0 = d4_coef(wP, wQ, I, base, fo, na, al);
    float cpv = c0.c / c0.b; // :77-78
    float dpv = c0.d / c0.b;
    cp[sbase] = cpv;
    dp[sbase] = dpv;
    for (int k0 = 1; k0 <= n - 2; k0 += D4_CH) { // :80-84
        D4Coef c[D4_CH];
#pragma unroll
        for (int u = 0; u < D4_CH; ++u) c[u] = d4_coef(wP, wQ, I, base + (size_t)min(k0 + u, n - 2) * stride, fo, na, al);
#pragma unroll
        for (int u = 0; u < D4_CH; ++u) {
            const int k = k0 + u;
            if (k <= n - 2) {
                const float temp = 1.0f / (c[u].b - c[u].a * cpv);
                cpv = c[u].c * temp;
                dpv = (c[u].d - c[u].a * dpv) * temp;
                cp[sbase + (size_t)k * sstride] = cpv;
                dp[sbase + (size_t)k * sstride] = dpv;
            }
        }
    }
    {
        const D4Coef cl = d4_coef(wP, wQ, I, base + (size_t)(n - 1) * stride, fo, na, al);
        dpv = (cl.d - cl.a * dpv) / (cl.b - cl.a * cpv); // :86
    }
    float x1 = dpv; // :89-92
    x[fo + base + (size_t)(n - 1) * stride] = x1;
    for (int k0 = n - 2; k0 >= 0; k0 -= D4_CH) {
        float cpk[D4_CH], dpk[D4_CH];
#pragma unroll
        for (int u = 0; u < D4_CH; ++u) {
            const int k = max(k0 - u, 0);
            cpk[u] = cp[sbase + (size_t)k * sstride];
            dpk[u] = dp[sbase + (size_t)k * sstride];
        }
#pragma unroll
        for (int u = 0; u < D4_CH; ++u) {
            const int k = k0 - u;
            if (k >= 0) {
                x1 = dpk[u] - cpk[u] * x1;
                x[fo + base + (size_t)k * stride] = x1;
            }
        }
    }
}

// Both line kinds of every channel in one grid, one wave per block.  blockIdx.y = channel; blockIdx.x < row_blocks: row lanes
// (row i; the longer chains at landscape shapes, dispatched first), else column lanes (column j).  The weight planes are
// [nrows x ncols], the channels and xc / xr / cp / dp [nrows x ncols x channels].  Row lanes: cp/dp share the image layout.
// Column lanes: cp/dp transposed (element i of column j at i*ncols + j) so that a wave's scratch traffic is one contiguous run.
__global__ void __launch_bounds__(D4_BLOCK) k_diff4_lines(const float *__restrict__ I, const float *__restrict__ wW,
                                                          const float *__restrict__ wN, const float *__restrict__ wE,
                                                          const float *__restrict__ wS, float *__restrict__ xc, float *__restrict__ xr,
                                                          float *__restrict__ cpc, float *__restrict__ dpc, float *__restrict__ cpr,
                                                          float *__restrict__ dpr, int nrows, int ncols, int row_blocks, float alpha)
{
    const size_t fo = (size_t)blockIdx.y * nrows * ncols;
    if ((int)blockIdx.x < row_blocks) {
        const int i = blockIdx.x * D4_BLOCK + threadIdx.x;
        if (i >= nrows) return;
        d4_line(wW, wE, I, xr, cpr, dpr, fo, (size_t)i, (size_t)nrows, fo + i, (size_t)nrows, ncols, -alpha, alpha);
    } else {
        const int j = ((int)blockIdx.x - row_blocks) * D4_BLOCK + threadIdx.x;
        if (j >= ncols) return;
        d4_line(wN, wS, I, xc, cpc, dpc, fo, (size_t)j * nrows, 1, fo + j, (size_t)ncols, nrows, -alpha, alpha);
    }
}

// Iout(:,:,k) = ver + hor (:60), n = nrows*ncols*channels elements.
__global__ void k_diff4_combine(const float *__restrict__ xc, const float *__restrict__ xr, float *__restrict__ Iout, size_t n)
{
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) Iout[p] = xc[p] + xr[p];
}

} // namespace diff
} // namespace pdeip
