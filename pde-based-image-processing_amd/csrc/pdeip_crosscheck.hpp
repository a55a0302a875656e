// pdeip_crosscheck.hpp -- kernels of the left-right check of two disparities and of the forward-backward check of two flows.
//
//   k_disp_crosscheck    one thread per pixel: the other view's disparity gathered at x + D0 (sym_warp_at), r = D0 + w, kept = |r| <= tol
//   k_flow_crosscheck    one thread per pixel: the backward flow sampled bilinearly at (x + Uf, y + Vf), the criterion of Sundaram, Brox
//                        and Keutzer (ECCV 2010)
//   k_crosscheck_final   the workgroups' partials folded into {kept, defined, mean, largest} by one workgroup of 1024 threads
//
// Thread mapping: that of PDEIP_PIXEL_INDEX (csrc/pdeip_pointwise.hpp) -- threadIdx.x runs down a MATLAB column, blockIdx.y is the
// column -- without its early return, because every lane takes part in the workgroup's sums.  For a smooth field a wave's gathers
// stay in a few columns, and the two row taps of the flow sample are adjacent in memory.
// All arithmetic is float64 on the promoted float32 inputs, FMA-free (-ffp-contract=off); results are rounded once to float32.
// Only scalar 4-byte loads and stores: a plane may start at any 4-byte offset.  The pixel kernels' workgroups are 256 threads (four
// waves of 64).
// No floating-point atomics: the sums are the library's fixed-order tree (csrc/pdeip_reduce.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "pdeip_bilinear.hpp"
#include "pdeip_reduce.hpp"
#include "pdeip_sym_warp.hpp"

namespace pdeip {
namespace crosscheck {

constexpr int BLOCK = 256;

__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double other = __shfl_xor(v, d, 64);
        if (other > v) v = other;
    }
    return v;
}

// The workgroup's {kept, defined, sum, largest (-1: none)}: the thread's value, the wave butterfly, the waves in ascending order.
// Thread q < 4 ends with quantity q and writes it to partials[q * nparts + part].  Every thread of the workgroup calls this.
__device__ __forceinline__ void fold_workgroup(double kept, double defined, double sum, double largest, double *__restrict__ partials,
                                               size_t nparts, size_t part)
{
    __shared__ double lds[4][BLOCK / 64];
    kept = wave_sum(kept);
    defined = wave_sum(defined);
    sum = wave_sum(sum);
    largest = wave_max(largest);
    const int wave = (int)threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        lds[0][wave] = kept;
        lds[1][wave] = defined;
        lds[2][wave] = sum;
        lds[3][wave] = largest;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int q = (int)threadIdx.x;
        double acc = lds[q][0];
#pragma unroll
        for (int w = 1; w < BLOCK / 64; w++) acc = (q == 3) ? (lds[q][w] > acc ? lds[q][w] : acc) : acc + lds[q][w];
        partials[(size_t)q * nparts + part] = acc;
    }
}

// Grid: pixel_grid(nrows, ncols, 1).  D0 is read at the thread's own pixel only (sparse_out may be D0); D1 is gathered and is never
// an output.  partials NULL (uniform over the grid): no statistics, no reduction.
__global__ __launch_bounds__(BLOCK) void k_disp_crosscheck(const float *D0, const float *__restrict__ D1, int nrows, int ncols, double tol,
                                                            float *sparse_out, float *__restrict__ mask_out, float *__restrict__ diff_out,
                                                            double *__restrict__ partials)
{
    const int i = (int)(blockIdx.x * BLOCK + threadIdx.x), j = (int)blockIdx.y;
    double kept = 0.0, defined = 0.0, sum = 0.0, largest = -1.0;
    if (i < nrows) {
        const size_t pos = (size_t)j * nrows + i;
        const float d0 = D0[pos];
        const double w = sym_warp_at(D1, d0, i, j, nrows, ncols);
        const double r = (double)d0 + w;
        const double mag = fabs(r);
        const bool def = isfinite(r), keep = def && mag <= tol;
        if (sparse_out != nullptr) sparse_out[pos] = keep ? d0 : __int_as_float(0x7fc00000);
        if (mask_out != nullptr) mask_out[pos] = keep ? 1.0f : 0.0f;
        if (diff_out != nullptr) diff_out[pos] = (float)r;
        if (def) {
            defined = 1.0;
            sum = mag;
            largest = mag;
            if (keep) kept = 1.0;
        }
    }
    if (partials != nullptr)
        fold_workgroup(kept, defined, sum, largest, partials, (size_t)gridDim.x * gridDim.y, (size_t)blockIdx.y * gridDim.x + blockIdx.x);
}

// Grid: pixel_grid(nrows, ncols, 1).  Needs nrows, ncols >= 2.  Ub, Vb are gathered and are never an output.
__global__ __launch_bounds__(BLOCK) void k_flow_crosscheck(const float *__restrict__ Uf, const float *__restrict__ Vf, const float *__restrict__ Ub,
                                                            const float *__restrict__ Vb, int nrows, int ncols, double a, double b,
                                                            float *__restrict__ mask_out, float *__restrict__ err_out, double *__restrict__ partials)
{
    const int i = (int)(blockIdx.x * BLOCK + threadIdx.x), j = (int)blockIdx.y;
    double kept = 0.0, defined = 0.0, sum = 0.0, largest = -1.0;
    if (i < nrows) {
        const size_t pos = (size_t)j * nrows + i;
        const double uf = (double)Uf[pos], vf = (double)Vf[pos];
        const double xq = (double)(j + 1) + uf, yq = (double)(i + 1) + vf;
        double ub = __longlong_as_double(0x7ff8000000000000LL), vb = ub;
        BilinearTaps T;
        if (bilinear_taps(xq, yq, nrows, ncols, &T)) { // csrc/pdeip_bilinear.hpp: the in-range rule and the clamps
            ub = bilinear(Ub, nrows, T);
            vb = bilinear(Vb, nrows, T);
        }
        const double ru = uf + ub, rv = vf + vb;
        const double e = ru * ru + rv * rv;
        const double lim = a * ((uf * uf + vf * vf) + (ub * ub + vb * vb)) + b;
        const bool def = isfinite(e), keep = def && e <= lim;
        const double err = sqrt(e);
        if (mask_out != nullptr) mask_out[pos] = keep ? 1.0f : 0.0f;
        if (err_out != nullptr) err_out[pos] = (float)err;
        if (def) {
            defined = 1.0;
            sum = err;
            largest = err;
            if (keep) kept = 1.0;
        }
    }
    if (partials != nullptr)
        fold_workgroup(kept, defined, sum, largest, partials, (size_t)gridDim.x * gridDim.y, (size_t)blockIdx.y * gridDim.x + blockIdx.x);
}

// One workgroup of FINAL_BLOCK threads.  Thread t folds partials t, t + 1024, .. in ascending order, then the same tree as within a
// workgroup: wave_sum, the sixteen waves in ascending order.  A single chain of dependent loads pays a load's latency per partial
// (a 4K call leaves 34 560 of them), so the loads of FINAL_BATCH steps are issued together and folded in their order afterwards:
// the additions and their order are those of the plain loop.  The counts are integers in doubles, exact below 2^53.
// stats = {kept, defined, sum / defined, largest}; with nothing defined the mean is 0/0 = NaN and so is the largest.
constexpr int FINAL_BLOCK = 1024;
constexpr int FINAL_BATCH = 4;

__global__ __launch_bounds__(FINAL_BLOCK) void k_crosscheck_final(const double *__restrict__ partials, int nparts, double *__restrict__ stats)
{
    __shared__ double lds[4][FINAL_BLOCK / 64];
    const double *__restrict__ pk = partials, *__restrict__ pd = partials + (size_t)nparts, *__restrict__ ps = partials + 2 * (size_t)nparts,
                 *__restrict__ pm = partials + 3 * (size_t)nparts;
    double kept = 0.0, defined = 0.0, sum = 0.0, largest = -1.0;
    int p = (int)threadIdx.x;
    for (; p < nparts - (FINAL_BATCH - 1) * FINAL_BLOCK; p += FINAL_BATCH * FINAL_BLOCK) {
        double k[FINAL_BATCH], d[FINAL_BATCH], s[FINAL_BATCH], m[FINAL_BATCH];
#pragma unroll
        for (int u = 0; u < FINAL_BATCH; u++) {
            k[u] = pk[p + u * FINAL_BLOCK];
            d[u] = pd[p + u * FINAL_BLOCK];
            s[u] = ps[p + u * FINAL_BLOCK];
            m[u] = pm[p + u * FINAL_BLOCK];
        }
#pragma unroll
        for (int u = 0; u < FINAL_BATCH; u++) {
            kept = kept + k[u];
            defined = defined + d[u];
            sum = sum + s[u];
            if (m[u] > largest) largest = m[u];
        }
    }
    for (; p < nparts; p += FINAL_BLOCK) {
        kept = kept + pk[p];
        defined = defined + pd[p];
        sum = sum + ps[p];
        if (pm[p] > largest) largest = pm[p];
    }
    kept = wave_sum(kept);
    defined = wave_sum(defined);
    sum = wave_sum(sum);
    largest = wave_max(largest);
    const int wave = (int)threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        lds[0][wave] = kept;
        lds[1][wave] = defined;
        lds[2][wave] = sum;
        lds[3][wave] = largest;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < FINAL_BLOCK / 64; w++) {
            kept = kept + lds[0][w];
            defined = defined + lds[1][w];
            sum = sum + lds[2][w];
            if (lds[3][w] > largest) largest = lds[3][w];
        }
        stats[0] = kept;
        stats[1] = defined;
        stats[2] = sum / defined;
        stats[3] = defined > 0.0 ? largest : __longlong_as_double(0x7ff8000000000000LL);
    }
}

} // namespace crosscheck
} // namespace pdeip
