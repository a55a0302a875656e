// pdeip_edt.hpp -- kernels of the exact Euclidean distance transform with its feature transform (which pixel is the nearest one), and of
// the three things that stand on it: the signed distance of a level set, the nearest-source fill of a sparse map, bwdist.
//
//   k_edt_cols        one workgroup per column (x frame): for every pixel the nearest feature within its own column, as the signed row
//                     offset g (feature row - own row) or G_NONE.  Two marches over the column in chunks of COL_BLOCK rows: top to bottom
//                     an inclusive prefix maximum of "row of the last feature at or above me", bottom to top an inclusive suffix minimum
//                     of "row of the first feature at or below me"; each chunk is a wave scan (__shfl_up / __shfl_down), the waves' totals
//                     meet in LDS, and a carry goes from chunk to chunk.  Of two equidistant features the upper one is kept.
//                     Bytes per pixel: 4 read (A) + 4 written (the prefix) + 4 read back + 4 written (g); the second pair hits L2, a
//                     column of a 4K frame being 8.6 KB.
//   k_edt_rows        one thread per pixel, lanes running down a column: candidates d^2 + g(i, j -+ d)^2 for d = 1, 2, ... outward, the best
//                     (d2, idx) pair kept in lexicographic order, until d^2 exceeds the best d2 (strictly: a candidate at j - d with g = 0
//                     ties at d^2 and has the lower index), d exceeds max_dist or both sides have left the frame.  A wave's reads of column
//                     j -+ d are contiguous.  Bytes per pixel: 4 per candidate read, 4 per output written; the candidates read are
//                     2 sqrt(d2) + 1 at most, so the work depends on the content.
//   k_sdf_combine     out = dist_to_outside - 0.5 on A >= 0, -(dist_to_inside - 0.5) elsewhere, one float32 subtraction
//   k_nearest_gather  out = the bits of D[idx], for any number of planes through one index plane or one per plane
//
// All arithmetic of the transform is integer: with both sides <= 32767, d^2 + g^2 <= 2 * 32766^2 < 2^31.  The tie rule -- among
// equidistant features the lowest linear index j nrows + i -- holds because the column pass hands each column's lowest-index nearest
// feature to the row pass, and the row pass minimises (d2, idx) over the columns.
// Only scalar 4-byte loads and stores: a plane may start at any 4-byte offset.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>

namespace pdeip {
namespace edt {

constexpr int COL_BLOCK = 256, COL_WAVES = COL_BLOCK / 64;
constexpr int ROW_BLOCK = 256;
constexpr int FLAT_BLOCK = 256;
constexpr unsigned MAX_UNITS = 1u << 20; // workgroups along x of the two transform kernels; beyond it they stride
constexpr int G_NONE = INT_MAX; // no feature in this column (within max_dist)
constexpr int D2_NONE = INT_MAX;
constexpr unsigned F32_INF = 0x7f800000u;

// PDEIP_EDT_*: bits 0-1 the predicate, bit 2 its complement.
__device__ __forceinline__ bool is_feature(float a, int mode)
{
    const int base = mode & 3;
    const bool f = base == 0 ? a > 0.0f : (base == 1 ? a >= 0.0f : a == a);
    return f != ((mode & 4) != 0);
}

// One column of one frame, by one workgroup.  base: the column's offset in A and G.
__device__ __forceinline__ void edt_column(const float *__restrict__ A, int *__restrict__ G, size_t base, int nrows, int mode, int max_dist,
                                           int *s_wave)
{
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const float *col = A + base;
    int *g = G + base;
    const int nchunks = (nrows + COL_BLOCK - 1) / COL_BLOCK;

    int carry = -1; // row of the last feature above this chunk
    for (int c = 0; c < nchunks; c++) {
        const int i = c * COL_BLOCK + t;
        int v = (i < nrows && is_feature(col[i], mode)) ? i : -1;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(v, off);
            if (lane >= off) v = max(v, o);
        }
        if (lane == 63) s_wave[wave] = v;
        __syncthreads();
        int up = carry, total = carry;
#pragma unroll
        for (int w = 0; w < COL_WAVES; w++) {
            const int sw = s_wave[w];
            if (w < wave) up = max(up, sw);
            total = max(total, sw);
        }
        if (i < nrows) g[i] = max(up, v);
        carry = total;
        __syncthreads(); // s_wave is rewritten by the next chunk
    }

    carry = INT_MAX; // row of the first feature below this chunk
    for (int c = nchunks - 1; c >= 0; c--) {
        const int i = c * COL_BLOCK + t;
        const int up = i < nrows ? g[i] : -1; // this thread's own store of the first march
        int v = (i < nrows && up == i) ? i : INT_MAX;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_down(v, off);
            if (lane + off < 64) v = min(v, o);
        }
        if (lane == 0) s_wave[wave] = v;
        __syncthreads();
        int down = carry, total = carry;
#pragma unroll
        for (int w = 0; w < COL_WAVES; w++) {
            const int sw = s_wave[w];
            if (w > wave) down = min(down, sw);
            total = min(total, sw);
        }
        down = min(down, v);
        if (i < nrows) {
            const int du = up >= 0 ? i - up : INT_MAX, dd = down != INT_MAX ? down - i : INT_MAX;
            int out = G_NONE;
            if (du != INT_MAX && du <= dd) out = -du; // the upper of two equidistant features
            else if (dd != INT_MAX) out = dd;
            if (max_dist > 0 && out != G_NONE && abs(out) > max_dist) out = G_NONE;
            g[i] = out;
        }
        carry = total;
        __syncthreads();
    }
}

// Grid: min(columns, MAX_UNITS) workgroups, a workgroup striding over the columns of all frames (column c of frame f is f * ncols + c,
// at offset (f * ncols + c) * nrows).  G like A.
__global__ __launch_bounds__(COL_BLOCK) void k_edt_cols(const float *__restrict__ A, int *__restrict__ G, int nrows, size_t columns, int mode,
                                                         int max_dist)
{
    __shared__ int s_wave[COL_WAVES];
    for (size_t c = blockIdx.x; c < columns; c += gridDim.x) edt_column(A, G, c * (size_t)nrows, nrows, mode, max_dist, s_wave);
}

// One pixel.  g: the frame's offsets; the outputs are the frame's.
__device__ __forceinline__ void edt_pixel(const int *__restrict__ g, int i, int j, int nrows, int ncols, int max_dist, int *__restrict__ d2_out,
                                          int *__restrict__ idx_out, float *__restrict__ dist_out)
{
    const int pos = j * nrows + i; // < 2^31: the frame has at most 2^31-1 pixels
    int best = D2_NONE, bidx = -1;
    const int g0 = g[pos];
    if (g0 != G_NONE) {
        best = g0 * g0;
        bidx = pos + g0;
    }
    int dmax = max(j, ncols - 1 - j);
    if (max_dist > 0) dmax = min(dmax, max_dist);
    for (int d = 1; d <= dmax; d++) {
        const int dd = d * d;
        if (dd > best) break;
        if (j - d >= 0) {
            const int p = pos - d * nrows, gl = g[p];
            if (gl != G_NONE) {
                const int c = dd + gl * gl, ci = p + gl;
                if (c < best || (c == best && ci < bidx)) {
                    best = c;
                    bidx = ci;
                }
            }
        }
        if (j + d < ncols) {
            const int p = pos + d * nrows, gr = g[p];
            if (gr != G_NONE) {
                const int c = dd + gr * gr, ci = p + gr;
                if (c < best || (c == best && ci < bidx)) {
                    best = c;
                    bidx = ci;
                }
            }
        }
    }
    if (max_dist > 0 && best != D2_NONE && (long long)best > (long long)max_dist * (long long)max_dist) {
        best = D2_NONE;
        bidx = -1;
    }
    if (d2_out != nullptr) d2_out[pos] = best;
    if (idx_out != nullptr) idx_out[pos] = bidx;
    if (dist_out != nullptr) dist_out[pos] = best == D2_NONE ? __uint_as_float(F32_INF) : (float)sqrt((double)best);
}

// Grid: (min(row blocks * frames, MAX_UNITS), ncols): blockIdx.y is the column, a workgroup strides over the units f * row_blocks + rb
// (ROW_BLOCK rows of frame f).  Every output may be null.
__global__ __launch_bounds__(ROW_BLOCK) void k_edt_rows(const int *__restrict__ G, int nrows, int ncols, int row_blocks, size_t units,
                                                         int max_dist, int *__restrict__ d2_out, int *__restrict__ idx_out,
                                                         float *__restrict__ dist_out)
{
    const int j = (int)blockIdx.y;
    const size_t n = (size_t)nrows * (size_t)ncols;
    for (size_t u = blockIdx.x; u < units; u += gridDim.x) {
        const size_t f = u / (size_t)row_blocks;
        const int i = (int)(u - f * (size_t)row_blocks) * ROW_BLOCK + (int)threadIdx.x;
        if (i >= nrows) continue;
        const size_t frame = f * n;
        edt_pixel(G + frame, i, j, nrows, ncols, max_dist, d2_out ? d2_out + frame : nullptr, idx_out ? idx_out + frame : nullptr,
                  dist_out ? dist_out + frame : nullptr);
    }
}

// Flat, grid-stride.  to_out: the distance of the inside pixels to the outside, to_in: of the outside pixels to the inside (each +Inf
// where there is none); none: the distance that stands for "none" (+Inf, or max_dist + 1 for a band).  out may be A.
__global__ __launch_bounds__(FLAT_BLOCK) void k_sdf_combine(const float *A, const float *__restrict__ to_out, const float *__restrict__ to_in,
                                                             float none, size_t n, float *out)
{
    const size_t stride = (size_t)gridDim.x * FLAT_BLOCK;
    for (size_t p = (size_t)blockIdx.x * FLAT_BLOCK + threadIdx.x; p < n; p += stride) {
        const bool inside = A[p] >= 0.0f;
        float d = inside ? to_out[p] : to_in[p];
        if (__float_as_uint(d) == F32_INF) d = none;
        const float m = d - 0.5f;
        out[p] = inside ? m : -m;
    }
}

// Flat, grid-stride over `planes` planes of n pixels.  idx: the feature transform of the planes' holes, one plane shared by all
// (idx_stride 0) or one per plane (idx_stride n); idx == own position on a known pixel, -1 where there is no source.
// out = the bits of D[idx]; without a source the pixel's own bits, or +0 with zero_none.  filled (null allowed) = 1 where a hole took a
// source's value.  dist (null allowed) passes through untouched: it is the transform's own output.  out may be D: a known pixel is
// then not stored, so nothing that is read is written.
__global__ __launch_bounds__(FLAT_BLOCK) void k_nearest_gather(const unsigned *D, const int *__restrict__ idx, size_t n, size_t idx_stride,
                                                                size_t total, int zero_none, unsigned *out, float *__restrict__ filled)
{
    const size_t stride = (size_t)gridDim.x * FLAT_BLOCK;
    for (size_t p = (size_t)blockIdx.x * FLAT_BLOCK + threadIdx.x; p < total; p += stride) {
        const size_t f = p / n, q = p - f * n;
        const int k = idx[f * idx_stride + q];
        const bool known = k == (int)q, has = k >= 0;
        if (!known) out[p] = has ? D[f * n + (size_t)k] : (zero_none ? 0u : D[p]);
        else if (out != D) out[p] = D[p];
        if (filled != nullptr) filled[p] = (has && !known) ? 1.0f : 0.0f;
    }
}

} // namespace edt
} // namespace pdeip
