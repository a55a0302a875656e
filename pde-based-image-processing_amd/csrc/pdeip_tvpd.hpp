// pdeip_tvpd.hpp -- kernels of primal-dual total variation (Chambolle and Pock's first-order iteration): TV-L1, ROF (TV-L2) and their
// Huber variants.  The recurrence is the contract of include/pdeip.h, float32 without contraction, restated by tests/tvpd_ref.py:
//
//   ub = (u + u) - u_prev;  q = p + sigma * grad(ub)  [/ (1 + sigma huber)];  p' = q / max(1, |q|);
//   v = u + tau * div(p');  u' = the data term's proximal step of v;  u_prev' = u
//
// grad is the forward difference (0 on the last row / column), div its negative adjoint (a missing north / west neighbour drops out).
// Every pixel of an iteration depends on the previous iterate alone, so nothing depends on the order of evaluation and both kernels
// give the same bits.
//
//   k_tvpd_step       one iteration per launch, one thread per pixel, lanes running down a column, frames on grid z.  A thread computes
//                     p' of its own pixel and recomputes px' of its north and py' of its west neighbour (seven values of ub, three of
//                     p: the repeated loads hit L1 / L2).  Reads u, u_prev, px, py, f; writes u', px', py' (u_prev' is the u it read).
//   k_tvpd_block<T>   T iterations per launch: a workgroup holds a TILE_R x TILE_C tile of u, ub, px, py, f in LDS with a halo of T pixels
//                     on every side and iterates on all of it.  A pixel's state after k iterations depends on nothing farther than k
//                     pixels away, so after T iterations everything T or more pixels inside the LDS region is exact; the rings nearer
//                     to a cut edge hold values that are never stored.  The border rules hold at the IMAGE border only; halo pixels
//                     outside the image are never computed or read.  Reads 5 planes and writes 4 per T iterations.
//
// px == nullptr: the dual variable is zero (the first launch of a call), nothing is read.  Only scalar 4-byte loads and stores: a plane
// may start at any 4-byte offset.  u and u_prev may be the same plane (the start); no output may be an input.
#pragma once
#include <hip/hip_runtime.h>

namespace pdeip {
namespace tvpd {

constexpr int BLOCK = 256;
// Rows (the contiguous direction) x columns of a blocked tile.  Chosen by measurement (tools/time_tvpd.py on a build with
// other values): the blocked kernel is paced by its arithmetic and its barriers, not by its bytes, so the small tile that lets
// several workgroups share a compute unit beats the large one that recomputes less.
#ifndef PDEIP_TVPD_TILE_R
#define PDEIP_TVPD_TILE_R 32
#endif
#ifndef PDEIP_TVPD_TILE_C
#define PDEIP_TVPD_TILE_C 16
#endif
constexpr int TILE_R = PDEIP_TVPD_TILE_R, TILE_C = PDEIP_TVPD_TILE_C;

// The call's constants, each formed once on the host in float32.
struct Consts {
    float sigma, tau;
    float tl;      // tau * lambda
    float onep_tl; // 1 + tl
    float hub_den; // 1 + sigma * huber
    int l2;        // the data term: 1 quadratic (ROF), 0 absolute (TV-L1)
    int huber;     // 1: divide q by hub_den
};

template <int T>
constexpr size_t block_lds_bytes() { return (size_t)5 * (TILE_R + 2 * T) * (TILE_C + 2 * T) * sizeof(float); }

// p' of one pixel from ub at the pixel, south and east of it (has_s / has_e: that neighbour exists in the image) and its p.
__device__ __forceinline__ void dual(float ubc, float ubs, float ube, bool has_s, bool has_e, float px, float py, const Consts &c, float &px_new,
                                     float &py_new)
{
    const float gx = has_s ? ubs - ubc : 0.0f, gy = has_e ? ube - ubc : 0.0f;
    float qx = px + c.sigma * gx, qy = py + c.sigma * gy;
    if (c.huber) {
        qx = qx / c.hub_den;
        qy = qy / c.hub_den;
    }
    const float s = sqrtf(qx * qx + qy * qy);
    const float n = s > 1.0f ? s : 1.0f; // a NaN norm divides by 1
    px_new = qx / n;
    py_new = qy / n;
}

// u' from v = u + tau * div p' and the data f (NaN: no data here).
__device__ __forceinline__ float primal(float v, float f, const Consts &c)
{
    if (f != f) return v;
    if (c.l2) return (v + c.tl * f) / c.onep_tl;
    const float r = v - f;
    return r > c.tl ? v - c.tl : (r < -c.tl ? v + c.tl : f);
}

// Grid: (ceil(nrows / BLOCK), ncols, frames).  PXo / PYo may be null (the last launch of a call).
__global__ __launch_bounds__(BLOCK) void k_tvpd_step(const float *U, const float *UP, const float *PX, const float *PY, const float *__restrict__ F,
                                                      int nrows, int ncols, Consts c, float *__restrict__ Uo, float *__restrict__ PXo,
                                                      float *__restrict__ PYo)
{
    const int i = (int)blockIdx.x * BLOCK + (int)threadIdx.x, j = (int)blockIdx.y;
    if (i >= nrows) return;
    const size_t pos = (size_t)blockIdx.z * ((size_t)nrows * (size_t)ncols) + (size_t)j * (size_t)nrows + (size_t)i;
    const size_t R = (size_t)nrows;
    const bool has_s = i + 1 < nrows, has_e = j + 1 < ncols, has_n = i > 0, has_w = j > 0, dual0 = PX == nullptr;
    const auto ub = [&](size_t p) {
        const float u = U[p];
        return (u + u) - UP[p];
    };
    const float u = U[pos];
    const float ubc = (u + u) - UP[pos];
    const float ubs = has_s ? ub(pos + 1) : 0.0f, ube = has_e ? ub(pos + R) : 0.0f;
    float px, py, pxn = 0.0f, pyw = 0.0f, unused;
    dual(ubc, ubs, ube, has_s, has_e, dual0 ? 0.0f : PX[pos], dual0 ? 0.0f : PY[pos], c, px, py);
    if (has_n) // the north neighbour's south is this pixel
        dual(ub(pos - 1), ubc, has_e ? ub(pos - 1 + R) : 0.0f, true, has_e, dual0 ? 0.0f : PX[pos - 1], dual0 ? 0.0f : PY[pos - 1], c, pxn, unused);
    if (has_w) // the west neighbour's east is this pixel
        dual(ub(pos - R), has_s ? ub(pos - R + 1) : 0.0f, ubc, has_s, true, dual0 ? 0.0f : PX[pos - R], dual0 ? 0.0f : PY[pos - R], c, unused, pyw);
    const float d = (has_n ? px - pxn : px) + (has_w ? py - pyw : py);
    const float v = u + c.tau * d;
    Uo[pos] = primal(v, F[pos], c);
    if (PXo != nullptr) {
        PXo[pos] = px;
        PYo[pos] = py;
    }
}

// Grid: (ceil(nrows / TILE_R), ceil(ncols / TILE_C), frames); dynamic LDS: block_lds_bytes<T>().  UPo / PXo / PYo may be null (the last
// launch of a call).
template <int T>
__global__ __launch_bounds__(BLOCK) void k_tvpd_block(const float *U, const float *UP, const float *PX, const float *PY,
                                                       const float *__restrict__ F, int nrows, int ncols, Consts c, float *__restrict__ Uo,
                                                       float *__restrict__ UPo, float *__restrict__ PXo, float *__restrict__ PYo)
{
    constexpr int LR = TILE_R + 2 * T, LC = TILE_C + 2 * T, LN = LR * LC;
    extern __shared__ float tvpd_lds[];
    float *sU = tvpd_lds, *sB = sU + LN, *sPX = sB + LN, *sPY = sPX + LN, *sF = sPY + LN;
    const int t = (int)threadIdx.x;
    const int gi0 = (int)blockIdx.x * TILE_R - T, gj0 = (int)blockIdx.y * TILE_C - T; // the LDS region's first row and column
    const size_t frame = (size_t)blockIdx.z * ((size_t)nrows * (size_t)ncols);
    const bool dual0 = PX == nullptr;

    // a pixel of the region: local index k = lj * LR + li; it exists if it lies inside the image
    for (int k = t; k < LN; k += BLOCK) {
        const int lj = k / LR, li = k - lj * LR, gi = gi0 + li, gj = gj0 + lj;
        float u = 0.0f, b = 0.0f, px = 0.0f, py = 0.0f, f = 0.0f;
        if (gi >= 0 && gi < nrows && gj >= 0 && gj < ncols) {
            const size_t p = frame + (size_t)gj * (size_t)nrows + (size_t)gi;
            u = U[p];
            b = (u + u) - UP[p];
            if (!dual0) {
                px = PX[p];
                py = PY[p];
            }
            f = F[p];
        }
        sU[k] = u;
        sB[k] = b;
        sPX[k] = px;
        sPY[k] = py;
        sF[k] = f;
    }
    __syncthreads();

#pragma unroll 1
    for (int it = 0; it < T; it++) {
        // the dual step: a neighbour beyond the region's edge counts as missing, which spoils one more ring per iteration
        for (int k = t; k < LN; k += BLOCK) {
            const int lj = k / LR, li = k - lj * LR, gi = gi0 + li, gj = gj0 + lj;
            if (gi < 0 || gi >= nrows || gj < 0 || gj >= ncols) continue;
            const bool has_s = gi + 1 < nrows && li + 1 < LR, has_e = gj + 1 < ncols && lj + 1 < LC;
            float px, py;
            dual(sB[k], has_s ? sB[k + 1] : 0.0f, has_e ? sB[k + LR] : 0.0f, has_s, has_e, sPX[k], sPY[k], c, px, py);
            sPX[k] = px;
            sPY[k] = py;
        }
        __syncthreads();
        // the primal step; the last one stores the tile
        for (int k = t; k < LN; k += BLOCK) {
            const int lj = k / LR, li = k - lj * LR, gi = gi0 + li, gj = gj0 + lj;
            if (gi < 0 || gi >= nrows || gj < 0 || gj >= ncols) continue;
            const bool has_n = gi > 0 && li > 0, has_w = gj > 0 && lj > 0;
            const float px = sPX[k], py = sPY[k], u = sU[k];
            const float d = (has_n ? px - sPX[k - 1] : px) + (has_w ? py - sPY[k - LR] : py);
            const float un = primal(u + c.tau * d, sF[k], c);
            if (it < T - 1) {
                sU[k] = un;
                sB[k] = (un + un) - u;
            } else if (li >= T && li < T + TILE_R && lj >= T && lj < T + TILE_C) {
                const size_t p = frame + (size_t)gj * (size_t)nrows + (size_t)gi;
                Uo[p] = un;
                if (UPo != nullptr) {
                    UPo[p] = u;
                    PXo[p] = px;
                    PYo[p] = py;
                }
            }
        }
        __syncthreads();
    }
}

} // namespace tvpd
} // namespace pdeip
