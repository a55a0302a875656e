// pdeip_flowviz.hpp -- kernels of flow2color (matlab/optical_flow/flow2color.m) and of the flow error measures.
//
//   k_flow_cell_init   the maximum's cell starts at "nothing seen"
//   k_flow_maxmag      max over the field of the non-NaN magnitudes sqrt(U^2 + V^2): per lane, wave butterfly, the workgroup's waves
//                      through LDS, one integer atomicMax per workgroup on the bit pattern (a maximum is exact: any order, same bits)
//   k_flow2color       one thread per pixel of the bordered picture: frame or interior, hsv -> rgb, float32 planes and / or uint8
//   k_flow_err_tiles   endpoint and angular error per pixel, the tile's count / sums / maximum in the library's fixed order
//   k_flow_err_final   the tile partials, staged through LDS, in ascending order, one thread per quantity; the four statistics
//
// All arithmetic is float64 on the promoted float32 inputs, FMA-free (-ffp-contract=off); results are rounded once to float32.
// Workgroups are 256 threads (four waves of 64).  No floating-point atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "pdeip_reduce.hpp"

namespace pdeip {
namespace flowviz {

constexpr int BLOCK = 256;
constexpr int TILE_SIDE = 16;            // k_flow2color: a workgroup colours a 16 x 16 tile of the bordered picture
constexpr int ERR_PER_THREAD = 8;        // k_flow_err_tiles: pixels per thread
constexpr int ERR_TILE = BLOCK * ERR_PER_THREAD;
constexpr int MAXMAG_BLOCKS = 1024;      // k_flow_maxmag: grid-stride beyond this many workgroups

constexpr double TWO_PI = 6.283185307179586;      // 2*pi as MATLAB evaluates it
constexpr double DEG_PER_RAD = 57.29577951308232; // 180/pi
constexpr double FRAME_MAX = 7.0710678118654755;  // sqrt(50): the frame field's largest magnitude, at its last pixel (5, 5)

// The cell holds (bit pattern of the largest non-negative double seen) + 1; 0: nothing seen.  Non-negative doubles order as their bit
// patterns do, Inf above every finite value.
__device__ __forceinline__ double cell_value(unsigned long long c)
{
    return c == 0ull ? __longlong_as_double(0x7ff8000000000000ll) : __longlong_as_double((long long)(c - 1ull));
}

__global__ void k_flow_cell_init(unsigned long long *cell)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) *cell = 0ull;
}

__device__ __forceinline__ unsigned long long mag_key(float uf, float vf, unsigned long long best)
{
    const double u = (double)uf, v = (double)vf;
    const double mag = sqrt(u * u + v * v);
    if (mag == mag) { // MATLAB's max ignores NaN
        const unsigned long long key = (unsigned long long)__double_as_longlong(mag) + 1ull;
        if (key > best) best = key;
    }
    return best;
}

// vec != 0: both planes are 16-byte aligned, the first n & ~3 pixels go as float4.
__global__ __launch_bounds__(BLOCK) void k_flow_maxmag(const float *__restrict__ U, const float *__restrict__ V, size_t n, int vec,
                                                        unsigned long long *cell)
{
    __shared__ unsigned long long wave_best[BLOCK / 64];
    const size_t stride = (size_t)gridDim.x * BLOCK, tid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    unsigned long long best = 0ull;
    size_t done = 0;
    if (vec) {
        const size_t n4 = n >> 2;
        const float4 *U4 = reinterpret_cast<const float4 *>(U), *V4 = reinterpret_cast<const float4 *>(V);
        for (size_t i = tid; i < n4; i += stride) {
            const float4 u = U4[i], v = V4[i];
            best = mag_key(u.x, v.x, best);
            best = mag_key(u.y, v.y, best);
            best = mag_key(u.z, v.z, best);
            best = mag_key(u.w, v.w, best);
        }
        done = n4 << 2;
    }
    for (size_t i = done + tid; i < n; i += stride) best = mag_key(U[i], V[i], best);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long other = __shfl_xor(best, d, 64);
        if (other > best) best = other;
    }
    if ((threadIdx.x & 63) == 0) wave_best[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < BLOCK / 64; w++)
            if (wave_best[w] > best) best = wave_best[w];
        if (best != 0ull) atomicMax(cell, best);
    }
}

// flow2color.m:38-59 for one pixel: dir = atan2(-v, -u) wrapped to turns, mag = |(u, v)| / maxv clamped at 1,
// valid = isfinite(u) & (mag <= 1), hsv = valid ? (dir, 1, mag) : (1, 0, 1); then the six-sector hsv2rgb.
__device__ __forceinline__ void flow_rgb(double u, double v, double maxv, double &r, double &g, double &b)
{
    double dir = atan2(-v, -u);
    if (dir < 0.0) dir = dir + TWO_PI;
    dir = dir / TWO_PI;
    double mag = sqrt(u * u + v * v) / maxv;
    if (mag > 1.0) mag = 1.0;
    const bool valid = isfinite(u) && (mag <= 1.0);
    const double h = valid ? dir : 1.0, s = valid ? 1.0 : 0.0, val = valid ? mag : 1.0;
    const double h6 = 6.0 * h;
    double kf = floor(h6);
    const double f = h6 - kf;
    if (kf >= 6.0) kf = 0.0;
    const int k = (int)kf;
    const double p = val * (1.0 - s), q = val * (1.0 - s * f), t = val * (1.0 - s * (1.0 - f));
    switch (k) {
    case 0: r = val; g = t; b = p; break;
    case 1: r = q; g = val; b = p; break;
    case 2: r = p; g = val; b = t; break;
    case 3: r = p; g = q; b = val; break;
    case 4: r = t; g = p; b = val; break;
    default: r = val; g = p; b = q; break;
    }
}

// uint8(round(255 x)) of the float32 picture: 255 x and the + 0.5 are exact in double, so this is MATLAB's round on x >= 0; saturating.
__device__ __forceinline__ unsigned char to_u8(float x)
{
    double y = floor(255.0 * (double)x + 0.5);
    y = y < 0.0 ? 0.0 : (y > 255.0 ? 255.0 : y);
    return (unsigned char)(int)y;
}

// Grid: (ceil(brows / 16), ceil(bcols / 16)); thread t colours row (t & 15), column (t >> 4) of its tile, so 16 lanes read 64
// contiguous bytes of a column of U, V and write as many of each rgb plane.  rgb8 is row-major interleaved: the tile's bytes pass
// through LDS and leave as 16 runs of 48 contiguous bytes, consecutive lanes writing consecutive bytes.
// maxgiven NaN: the maximum is read from `cell` (k_flow_maxmag ran before on the same stream).
// The flow sits at 0-based offset border - 1 of the bordered picture (flow2color.m:66 indexes from `border`, 1-based).
__global__ __launch_bounds__(BLOCK) void k_flow2color(const float *__restrict__ U, const float *__restrict__ V, int nrows, int ncols, int border,
                                                       double maxgiven, const unsigned long long *cell, float *__restrict__ rgb,
                                                       unsigned char *__restrict__ rgb8, double *maxvalue_out)
{
    __shared__ unsigned char tile8[TILE_SIDE][TILE_SIDE * 3];
    const int brows = nrows + 2 * border, bcols = ncols + 2 * border;
    const int i0 = (int)blockIdx.x * TILE_SIDE, j0 = (int)blockIdx.y * TILE_SIDE;
    const int ti = (int)threadIdx.x & (TILE_SIDE - 1), tj = (int)threadIdx.x / TILE_SIDE;
    const int i = i0 + ti, j = j0 + tj;
    const double maxv = (maxgiven == maxgiven) ? maxgiven : cell_value(*cell);
    if (maxvalue_out != nullptr && threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0) *maxvalue_out = maxv;
    if (i < brows && j < bcols) {
        const int off = border > 0 ? border - 1 : 0;
        const int fi = i - off, fj = j - off;
        double r, g, b;
        if (fi >= 0 && fi < nrows && fj >= 0 && fj < ncols) {
            const size_t at = (size_t)fj * nrows + fi;
            flow_rgb((double)U[at], (double)V[at], maxv, r, g, b);
        } else {
            const double X = ((double)(j + 1) / (double)bcols - 0.5) * 10.0, Y = ((double)(i + 1) / (double)brows - 0.5) * 10.0;
            flow_rgb(X, Y, FRAME_MAX, r, g, b);
        }
        const float rf = (float)r, gf = (float)g, bf = (float)b;
        if (rgb != nullptr) {
            const size_t plane = (size_t)brows * bcols, at = (size_t)j * brows + i;
            rgb[at] = rf;
            rgb[plane + at] = gf;
            rgb[2 * plane + at] = bf;
        }
        if (rgb8 != nullptr) {
            tile8[ti][3 * tj] = to_u8(rf);
            tile8[ti][3 * tj + 1] = to_u8(gf);
            tile8[ti][3 * tj + 2] = to_u8(bf);
        }
    }
    if (rgb8 != nullptr) { // uniform over the grid
        __syncthreads();
        const int wide = (bcols - j0 < TILE_SIDE ? bcols - j0 : TILE_SIDE) * 3;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int byte = (int)threadIdx.x + k * BLOCK, row = byte / (TILE_SIDE * 3), col = byte % (TILE_SIDE * 3);
            if (i0 + row < brows && col < wide) rgb8[((size_t)(i0 + row) * bcols + j0) * 3 + col] = tile8[row][col];
        }
    }
}

// One workgroup per tile of ERR_TILE pixels; thread t takes pixels tile * ERR_TILE + k * 256 + t, k ascending.  A pixel counts when U, V,
// Ut, Vt are finite there and mask (when given) is nonzero.  partials: [4][ntiles] doubles -- count, sum of endpoint errors, sum of
// angular errors, largest endpoint error (-1: none) -- each the thread's value, wave_sum, the waves in ascending order.
__global__ __launch_bounds__(BLOCK) void k_flow_err_tiles(const float *__restrict__ U, const float *__restrict__ V, const float *__restrict__ Ut,
                                                           const float *__restrict__ Vt, const float *__restrict__ mask, size_t n,
                                                           float *__restrict__ epe_out, float *__restrict__ ang_out, double *__restrict__ partials)
{
    __shared__ double lds[4][BLOCK / 64];
    const size_t base = (size_t)blockIdx.x * ERR_TILE + threadIdx.x;
    double cnt = 0.0, se = 0.0, sa = 0.0, me = -1.0;
#pragma unroll
    for (int k = 0; k < ERR_PER_THREAD; k++) {
        const size_t at = base + (size_t)k * BLOCK;
        if (at >= n) break;
        const double u = (double)U[at], v = (double)V[at], ut = (double)Ut[at], vt = (double)Vt[at];
        const bool counted = isfinite(u) && isfinite(v) && isfinite(ut) && isfinite(vt) && (mask == nullptr || mask[at] != 0.0f);
        float ef = __int_as_float(0x7fc00000), af = ef;
        if (counted) {
            const double du = u - ut, dv = v - vt;
            const double epe = sqrt(du * du + dv * dv);
            double c = (u * ut + v * vt + 1.0) / (sqrt(u * u + v * v + 1.0) * sqrt(ut * ut + vt * vt + 1.0));
            c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
            const double ang = acos(c) * DEG_PER_RAD;
            cnt = cnt + 1.0;
            se = se + epe;
            sa = sa + ang;
            if (epe > me) me = epe;
            ef = (float)epe;
            af = (float)ang;
        }
        if (epe_out != nullptr) epe_out[at] = ef;
        if (ang_out != nullptr) ang_out[at] = af;
    }
    cnt = wave_sum(cnt);
    se = wave_sum(se);
    sa = wave_sum(sa);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double other = __shfl_xor(me, d, 64);
        if (other > me) me = other;
    }
    const int wave = (int)threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        lds[0][wave] = cnt;
        lds[1][wave] = se;
        lds[2][wave] = sa;
        lds[3][wave] = me;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int q = (int)threadIdx.x;
        double acc = lds[q][0];
#pragma unroll
        for (int w = 1; w < BLOCK / 64; w++) acc = (q == 3) ? (lds[q][w] > acc ? lds[q][w] : acc) : acc + lds[q][w];
        partials[(size_t)q * gridDim.x + blockIdx.x] = acc;
    }
}

// One workgroup.  The tile partials come in 256 at a time, one coalesced load per thread and quantity, and wait in LDS; one thread per
// quantity folds it over them in ascending tile order (a tile past the last one counts as 0, or as "none" for the maximum, which
// changes no bit: the sums are non-negative).  A single thread reading the partials from memory pays a load's latency per tile.
// stats = {count, mean endpoint error, mean angular error, largest endpoint error}; with no counted pixel the means are 0/0 = NaN
// and so is the maximum.
__global__ __launch_bounds__(BLOCK) void k_flow_err_final(const double *__restrict__ partials, int ntiles, double *__restrict__ stats)
{
    __shared__ double stage[4][BLOCK];
    __shared__ double total[4];
    // the three sums fold on lanes 0..2 of wave 0, the maximum on lane 0 of wave 1: each chain is one dependent operation per tile
    const int q = threadIdx.x < 3 ? (int)threadIdx.x : (threadIdx.x == 64 ? 3 : -1);
    double acc = (q == 3) ? -1.0 : 0.0;
    for (int base = 0; base < ntiles; base += BLOCK) {
        const int t = base + (int)threadIdx.x;
#pragma unroll
        for (int k = 0; k < 4; k++) stage[k][threadIdx.x] = t < ntiles ? partials[(size_t)k * ntiles + t] : (k == 3 ? -1.0 : 0.0);
        __syncthreads();
        if (q == 3) {
#pragma unroll 16
            for (int k = 0; k < BLOCK; k++) acc = stage[3][k] > acc ? stage[3][k] : acc;
        } else if (q >= 0) {
#pragma unroll 16
            for (int k = 0; k < BLOCK; k++) acc = acc + stage[q][k];
        }
        __syncthreads();
    }
    if (q >= 0) total[q] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double cnt = total[0];
        stats[0] = cnt;
        stats[1] = total[1] / cnt;
        stats[2] = total[2] / cnt;
        stats[3] = cnt > 0.0 ? total[3] : __longlong_as_double(0x7ff8000000000000ll);
    }
}

} // namespace flowviz
} // namespace pdeip
