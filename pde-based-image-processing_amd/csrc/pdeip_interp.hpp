// pdeip_interp.hpp -- kernels of the motion-compensated frame interpolation: the flow of frame 0 -> 1 carried forward to time t (a
// scatter with conflicts) and the occlusion-aware blend of the two frames along it.
//
//   k_splat_clear     the key plane set to all ones (flat, grid-stride)
//   k_flow_splat      one thread per source pixel: its cost, its landing point, atomicMin of (bits(cost) << 32 | index) on the one,
//                     two or four targets around it
//   k_splat_resolve   one thread per target: the winner's flow with its own bits, NaN where nothing landed
//   k_interp_blend    one thread per pixel: both frames sampled along the flow at t, the table of include/pdeip.h; the channels are a
//                     loop inside the thread, so the positions are computed once
//
// Thread mapping of the pixel kernels: PDEIP_PIXEL_INDEX's (csrc/pdeip_pointwise.hpp) -- threadIdx.x runs down a MATLAB column,
// blockIdx.y is the column -- in workgroups of 256 threads.
// All arithmetic is float64 on the promoted float32 inputs, FMA-free (-ffp-contract=off); results are rounded once to float32.
// Only scalar 4-byte loads and stores on the float planes: a plane may start at any 4-byte offset.  The key plane is the library's
// own (WS_INTERP) and 8-byte aligned.
// The only atomics are 64-bit unsigned integer minima, so the winner of a target does not depend on the order of arrival.
#pragma once
#include <hip/hip_runtime.h>

#include "pdeip_bilinear.hpp"

namespace pdeip {
namespace interp {

constexpr int BLOCK = 256;
constexpr unsigned long long KEY_EMPTY = ~0ULL;
constexpr unsigned F32_QNAN = 0x7fc00000u, F32_INF = 0x7f800000u;

__global__ __launch_bounds__(BLOCK) void k_splat_clear(unsigned long long *__restrict__ keys, size_t n)
{
    const size_t stride = (size_t)gridDim.x * BLOCK;
    for (size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x; p < n; p += stride) keys[p] = KEY_EMPTY;
}

// Grid: pixel_grid(nrows, ncols, 1).  I0, I1 [nrows x ncols x channels] or both NULL (cost 0).  keys [nrows x ncols], cleared.
__global__ __launch_bounds__(BLOCK) void k_flow_splat(const float *__restrict__ Uf, const float *__restrict__ Vf, const float *__restrict__ I0,
                                                       const float *__restrict__ I1, int channels, int nrows, int ncols, double t,
                                                       unsigned long long *__restrict__ keys)
{
    const int i = (int)(blockIdx.x * BLOCK + threadIdx.x), j = (int)blockIdx.y;
    if (i >= nrows) return;
    const size_t pos = (size_t)j * nrows + i;
    const float uf32 = Uf[pos], vf32 = Vf[pos];
    if (!isfinite(uf32) || !isfinite(vf32)) return; // not a source
    const double uf = (double)uf32, vf = (double)vf32, x = (double)(j + 1), y = (double)(i + 1);
    unsigned cbits = 0u;
    if (I0 != nullptr) {
        cbits = F32_INF;
        BilinearTaps T;
        if (bilinear_taps(x + uf, y + vf, nrows, ncols, &T)) {
            const size_t n = (size_t)nrows * ncols;
            double sum = 0.0;
            for (int ch = 0; ch < channels; ch++) {
                const double b = bilinear(I1 + (size_t)ch * n, nrows, T);
                sum = sum + fabs((double)I0[(size_t)ch * n + pos] - b);
            }
            const float c = (float)sum;
            if (c == c) cbits = __float_as_uint(c); // a NaN sum keeps +Inf; c >= +0 otherwise
        }
    }
    const unsigned long long key = ((unsigned long long)cbits << 32) | (unsigned long long)(unsigned)pos;
    const double xq = x + t * uf, yq = y + t * vf;
    const double fx = floor(xq), fy = floor(yq);
    const int nx = (xq != fx) ? 2 : 1, ny = (yq != fy) ? 2 : 1;
    for (int a = 0; a < nx; a++) {
        const double col = fx + (double)a; // 1-based; compared as a double, a far landing never becomes an int
        if (!(col >= 1.0 && col <= (double)ncols)) continue;
        const size_t cbase = (size_t)((int)col - 1) * nrows;
        for (int b = 0; b < ny; b++) {
            const double row = fy + (double)b;
            if (!(row >= 1.0 && row <= (double)nrows)) continue;
            atomicMin(&keys[cbase + (size_t)((int)row - 1)], key);
        }
    }
}

// Grid: pixel_grid(nrows, ncols, 1).  Uf, Vf are gathered and are never an output.  cost_out NULL allowed.
__global__ __launch_bounds__(BLOCK) void k_splat_resolve(const unsigned long long *__restrict__ keys, const float *__restrict__ Uf,
                                                          const float *__restrict__ Vf, int nrows, int ncols, float *__restrict__ Ut_out,
                                                          float *__restrict__ Vt_out, float *__restrict__ cost_out)
{
    const int i = (int)(blockIdx.x * BLOCK + threadIdx.x), j = (int)blockIdx.y;
    if (i >= nrows) return;
    const size_t pos = (size_t)j * nrows + i;
    const unsigned long long key = keys[pos];
    unsigned ub = F32_QNAN, vb = F32_QNAN, cb = F32_QNAN;
    if (key != KEY_EMPTY) {
        const size_t p = (size_t)(key & 0xffffffffULL); // < nrows * ncols: only sources of this frame wrote keys
        ub = __float_as_uint(Uf[p]);
        vb = __float_as_uint(Vf[p]);
        cb = (unsigned)(key >> 32);
    }
    Ut_out[pos] = __uint_as_float(ub);
    Vt_out[pos] = __uint_as_float(vb);
    if (cost_out != nullptr) cost_out[pos] = __uint_as_float(cb);
}

// The mask value at the sample's nearest pixel: column min(floor(xq + 0.5), ncols), row alike (1-based); (xq, yq) is in range.
__device__ __forceinline__ bool mask_at(const float *__restrict__ M, double xq, double yq, int nrows, int ncols)
{
    if (M == nullptr) return true;
    double c = floor(xq + 0.5), r = floor(yq + 0.5);
    if (c > (double)ncols) c = (double)ncols;
    if (r > (double)nrows) r = (double)nrows;
    return M[(size_t)((int)c - 1) * nrows + (size_t)((int)r - 1)] != 0.0f;
}

// Grid: pixel_grid(nrows, ncols, 1).  tq = 1 - t, formed on the host.  M0, M1 both given or both NULL; source_out NULL allowed.
__global__ __launch_bounds__(BLOCK) void k_interp_blend(const float *__restrict__ I0, const float *__restrict__ I1, int channels,
                                                         const float *__restrict__ Ut, const float *__restrict__ Vt, const float *__restrict__ M0,
                                                         const float *__restrict__ M1, int nrows, int ncols, double t, double tq,
                                                         float *__restrict__ It_out, float *__restrict__ source_out)
{
    const int i = (int)(blockIdx.x * BLOCK + threadIdx.x), j = (int)blockIdx.y;
    if (i >= nrows) return;
    const size_t pos = (size_t)j * nrows + i, n = (size_t)nrows * ncols;
    const float u32 = Ut[pos], v32 = Vt[pos];
    const bool fin = isfinite(u32) && isfinite(v32);
    const double u = (double)u32, v = (double)v32, x = (double)(j + 1), y = (double)(i + 1);
    const double x0 = x - t * u, y0 = y - t * v, x1 = x + tq * u, y1 = y + tq * v;
    BilinearTaps T0, T1;
    const bool r0 = fin && bilinear_taps(x0, y0, nrows, ncols, &T0);
    const bool r1 = fin && bilinear_taps(x1, y1, nrows, ncols, &T1);
    int src = 0; // 0 neither, 1 frame 0, 2 frame 1, 3 both
    if (r0 && r1) {
        const bool p0 = mask_at(M0, x0, y0, nrows, ncols), p1 = mask_at(M1, x1, y1, nrows, ncols);
        // the sample that fails its own view's check shows what only that view sees; the one that passes there is the occluder
        src = (p0 == p1) ? 3 : (p0 ? 2 : 1);
    } else if (r0) {
        src = 1;
    } else if (r1) {
        src = 2;
    }
    if (source_out != nullptr) source_out[pos] = (float)src;
    for (int ch = 0; ch < channels; ch++) {
        const size_t off = (size_t)ch * n;
        float out = __uint_as_float(F32_QNAN);
        if (src == 1) {
            out = (float)bilinear(I0 + off, nrows, T0);
        } else if (src == 2) {
            out = (float)bilinear(I1 + off, nrows, T1);
        } else if (src == 3) {
            const double a0 = bilinear(I0 + off, nrows, T0), a1 = bilinear(I1 + off, nrows, T1);
            out = (float)(tq * a0 + t * a1);
        }
        It_out[off + pos] = out;
    }
}

} // namespace interp
} // namespace pdeip
