// pdeip_diffusion.hpp -- the nonlinear (lagged-diffusivity) diffusion filter matlab/diffusion/Diffusion4_v10.m: the line solves
// of one outer iteration and the combine that ends it.  The weights are the DdiffWeights kernel (k_diffweights6,
// csrc/pdeip_pointwise.hpp) with eps = 0.00001f and the channels as its frames, in its <true> form: the maximum over the channels
// omits a NaN of any channel, as the .m's max(w, [], 3).
//
// One outer iteration (Diffusion4_v10.m:44-62), every channel k of Iout solved independently with the iteration's weights:
//   ver = TDMA(-alpha*wN, 2 + alpha*(wN + wS), -alpha*wS, Iout(:,:,k))     along every column
//   hor = TDMA(-alpha*wW, 2 + alpha*(wW + wE), -alpha*wE, Iout(:,:,k))     along every row
//   Iout(:,:,k) = ver + hor
// alpha is the single the double parameter rounds to.  TDMA (:70-92) is the line solve of pdeip_thomas.hpp: forward (:77-86),
// then the plain back-substitution (:89-92).  Both solves read the iteration's input, so the column lanes and the row lanes run
// side by side in one launch (k_diff4_lines) and a second, elementwise launch (k_diff4_combine) adds them.
// -ffp-contract=off (build.py) keeps every product and sum separate.
#pragma once
#include "pdeip_thomas.hpp"

namespace pdeip {
namespace diff {

// a, b, c, d of the element at weight-plane position wpos: wP is the weight towards the previous element of the line (wN for a
// column, wW for a row), wQ the one towards the next (wS, wE); d is the channel's value there.  na = -alpha, al = alpha.
__device__ __forceinline__ thomas::Coef d4_coef(const float *__restrict__ wP, const float *__restrict__ wQ,
                                                const float *__restrict__ I, size_t wpos, size_t fo, float na, float al)
{
    const float p = wP[wpos], q = wQ[wpos];
    thomas::Coef r;
    r.a = na * p;
    r.b = 2.0f + al * (p + q);
    r.c = na * q;
    r.d = I[fo + wpos];
    return r;
}

// One Thomas solve of a line L of a weight plane (a Line of frame offset 0) for the channel at fo: the channel's elements, x and
// cp/dp sit fo further on.
__device__ __forceinline__ void d4_line(const float *__restrict__ wP, const float *__restrict__ wQ, const float *__restrict__ I,
                                        float *__restrict__ x, float *__restrict__ cp, float *__restrict__ dp, size_t fo,
                                        thomas::Line L, float na, float al)
{
    auto coef_at = [&](int k) __attribute__((always_inline)) { return d4_coef(wP, wQ, I, L.base + (size_t)k * L.stride, fo, na, al); };
    auto store = [&](int k, float v) __attribute__((always_inline)) { x[fo + L.base + (size_t)k * L.stride] = v; };
    thomas::back_plain(cp, dp, fo + L.sbase, L.sstride, L.n, thomas::forward(coef_at, cp, dp, fo + L.sbase, L.sstride, L.n), store);
}

// Both line kinds of every channel in one grid (thomas::lane_of), blockIdx.y = channel.  The weight planes are [nrows x ncols],
// the channels and xc / xr / cp / dp [nrows x ncols x channels].
__global__ void __launch_bounds__(thomas::BLOCK) k_diff4_lines(const float *__restrict__ I, const float *__restrict__ wW,
                                                               const float *__restrict__ wN, const float *__restrict__ wE,
                                                               const float *__restrict__ wS, float *__restrict__ xc,
                                                               float *__restrict__ xr, float *__restrict__ cpc, float *__restrict__ dpc,
                                                               float *__restrict__ cpr, float *__restrict__ dpr, int nrows, int ncols,
                                                               int row_blocks, float alpha)
{
    const size_t fo = (size_t)blockIdx.y * nrows * ncols;
    const thomas::Lane l = thomas::lane_of(blockIdx.x, row_blocks, nrows, ncols);
    if (l.kind == thomas::ROW)
        d4_line(wW, wE, I, xr, cpr, dpr, fo, thomas::row_line(0, l.idx, nrows, ncols), -alpha, alpha);
    else if (l.kind == thomas::COL)
        d4_line(wN, wS, I, xc, cpc, dpc, fo, thomas::col_line(0, l.idx, nrows, ncols), -alpha, alpha);
}

// Iout(:,:,k) = ver + hor (:60), n = nrows*ncols*channels elements.
__global__ void k_diff4_combine(const float *__restrict__ xc, const float *__restrict__ xr, float *__restrict__ Iout, size_t n)
{
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) Iout[p] = xc[p] + xr[p];
}

} // namespace diff
} // namespace pdeip
