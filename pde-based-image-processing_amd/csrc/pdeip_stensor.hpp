// pdeip_stensor.hpp -- kernels of structure-tensor anisotropic diffusion (Weickert's EED and CED): a separable Gaussian of a
// chosen scale, the structure tensor, and the diffusion tensor with the eight stencil weights of div(D grad u), ready for
// pdeip_pde_sor8_dev / pdeip_pde_alr8_dev.  Host side: pdeip_stensor.hip; contract: include/pdeip.h; restatement the tests compare
// with: tests/stensor_ref.py.  Planes are column-major [frames][ncols][nrows], the row index contiguous.
#pragma once
#include <hip/hip_runtime.h>

#include "pdeip_pointwise.hpp"
#include "pdeip_tensor8.hpp"

namespace pdeip {
namespace st {

// ---- Gaussian smoothing --------------------------------------------------------------------------------------------------
// out(p) = ((g[0] x[p-R] + g[1] x[p-R+1]) + ...) + g[2R] x[p+R] along one axis, indices clamped to the frame ('replicate'), single,
// left to right.  Both passes stage their input in LDS once, so a pass reads an element from global memory (T + 2R) / T times
// (T = GAUSS_T, the tile edge along the filtered axis), not 2R + 1 times; the halo's re-reads are the neighbouring workgroup's
// tile and come from L2.  A workgroup is GAUSS_WAVES waves of 64 lanes, the lanes along the contiguous row index in both passes.
constexpr int GAUSS_RMAX = 32, GAUSS_T = 64, GAUSS_WAVES = 4;
struct GaussTaps {
    float g[2 * GAUSS_RMAX + 1];
    int R;
};

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// Along the rows (down a column).  Workgroup: GAUSS_T rows of GAUSS_WAVES columns, one column per wave; tile[wave] holds the
// wave's GAUSS_T rows and R rows either side.  Grid: (ceil(nrows / GAUSS_T), ceil(ncols / GAUSS_WAVES), frames).
__global__ void __launch_bounds__(GAUSS_T *GAUSS_WAVES) k_gauss_rows(float *out, const float *in, GaussTaps T, int nrows, int ncols)
{
    __shared__ float tile[GAUSS_WAVES][GAUSS_T + 2 * GAUSS_RMAX];
    __shared__ float g[2 * GAUSS_RMAX + 1];
    const int R = T.R, x = threadIdx.x, y = threadIdx.y, tid = y * GAUSS_T + x;
    if (tid <= 2 * R) g[tid] = T.g[tid];
    const int i0 = blockIdx.x * GAUSS_T, j = blockIdx.y * GAUSS_WAVES + y;
    const size_t base = (size_t)blockIdx.z * nrows * ncols + (size_t)j * nrows;
    if (j < ncols)
        for (int e = x; e < GAUSS_T + 2 * R; e += GAUSS_T) tile[y][e] = in[base + clampi(i0 - R + e, nrows - 1)];
    __syncthreads();
    const int i = i0 + x;
    if (j >= ncols || i >= nrows) return;
    float acc = g[0] * tile[y][x];
    for (int k = 1; k <= 2 * R; k++) acc = acc + g[k] * tile[y][x + k];
    out[base + i] = acc;
}

// Along the columns.  Workgroup: GAUSS_T rows x GAUSS_T columns; the dynamic LDS holds the (GAUSS_T + 2R) column strips of
// GAUSS_T rows the tile's outputs read ((GAUSS_T + 2R) x GAUSS_T floats, at most 32 KiB), a wave loads and later computes every
// GAUSS_WAVES-th strip.  Grid: (ceil(nrows / GAUSS_T), ceil(ncols / GAUSS_T), frames).
__global__ void __launch_bounds__(GAUSS_T *GAUSS_WAVES) k_gauss_cols(float *out, const float *in, GaussTaps T, int nrows, int ncols)
{
    extern __shared__ float strips[]; // [GAUSS_T + 2R][GAUSS_T]
    __shared__ float g[2 * GAUSS_RMAX + 1];
    const int R = T.R, x = threadIdx.x, y = threadIdx.y, tid = y * GAUSS_T + x;
    if (tid <= 2 * R) g[tid] = T.g[tid];
    const int i0 = blockIdx.x * GAUSS_T, j0 = blockIdx.y * GAUSS_T, i = i0 + x;
    const size_t base = (size_t)blockIdx.z * nrows * ncols;
    const int il = i < nrows ? i : nrows - 1; // lanes past the last row load it again and store nothing
    for (int c = y; c < GAUSS_T + 2 * R; c += GAUSS_WAVES)
        strips[c * GAUSS_T + x] = in[base + (size_t)clampi(j0 - R + c, ncols - 1) * nrows + il];
    __syncthreads();
    if (i >= nrows) return;
    for (int c = y; c < GAUSS_T && j0 + c < ncols; c += GAUSS_WAVES) {
        float acc = g[0] * strips[c * GAUSS_T + x];
        for (int k = 1; k <= 2 * R; k++) acc = acc + g[k] * strips[(c + k) * GAUSS_T + x];
        out[base + (size_t)(j0 + c) * nrows + i] = acc;
    }
}

// ---- structure tensor ------------------------------------------------------------------------------------------------------
// J11 = sum_c gx^2, J12 = sum_c gx gy, J22 = sum_c gy^2 of the channels of V [nrows x ncols x channels] (Weickert's joint tensor of
// a colour image), single, the channels added in index order onto the first channel's product.  gx (toward increasing column)
// and gy (toward increasing row) are the Alvarez 3x3 derivative with 'replicate' borders: the three differences across the
// pixel first, then (w1 d- + w2 d0) + w1 d+ with w1 = 1 / (4 + sqrt 8), w2 = sqrt 2 / (4 + sqrt 8) as singles (rounded on the host).
// The derivatives stay in registers.
__global__ void k_st_products(float *J11, float *J12, float *J22, const float *V, int nrows, int ncols, int channels, float w1, float w2)
{
    PDEIP_PIXEL_INDEX();
    const size_t n = (size_t)nrows * ncols;
    const int im = i > 0 ? i - 1 : 0, ip = i < nrows - 1 ? i + 1 : i, jm = j > 0 ? j - 1 : 0, jp = j < ncols - 1 ? j + 1 : j;
    float a11 = 0.0f, a12 = 0.0f, a22 = 0.0f;
    for (int c = 0; c < channels; ++c) {
        const float *P = V + (size_t)c * n;
        auto at = [&](int ii, int jj) { return P[(size_t)jj * nrows + ii]; };
        const float mm = at(im, jm), m0 = at(im, j), mp = at(im, jp), zm = at(i, jm), zp = at(i, jp), pm = at(ip, jm), p0 = at(ip, j), pp = at(ip, jp);
        const float gx = (w1 * (mp - mm) + w2 * (zp - zm)) + w1 * (pp - pm); // rows i-1, i, i+1
        const float gy = (w1 * (pm - mm) + w2 * (p0 - m0)) + w1 * (pp - mp); // columns j-1, j, j+1
        const float p11 = gx * gx, p12 = gx * gy, p22 = gy * gy;
        a11 = c == 0 ? p11 : a11 + p11;
        a12 = c == 0 ? p12 : a12 + p12;
        a22 = c == 0 ? p22 : a22 + p22;
    }
    J11[pos] = a11;
    J12[pos] = a12;
    J22[pos] = a22;
}

// ---- diffusion tensor and the eight weights --------------------------------------------------------------------------------
struct TensorRule {
    int ced;                 // 0: edge-enhancing, 1: coherence-enhancing
    double lambda, alpha, C; // EED's contrast; CED's floor and threshold
};

// D = lambda1 e1 e1' + lambda2 e2 e2' with e1 the eigenvector of J's larger eigenvalue mu1 (across the structure), in double from
// the single J; every operation in the order written (include/pdeip.h).  A NaN in J fails every `> 0`: c2 = 1, s2 = 0 and the
// eigenvalues of a flat pixel.
__device__ __forceinline__ void diffusion_tensor(double j11, double j12, double j22, const TensorRule &p, double &D11, double &D22, double &D12)
{
    const double s = j11 + j22, d = j11 - j22, r = sqrt(d * d + 4.0 * j12 * j12), mu1 = 0.5 * (s + r);
    const double c2 = r > 0.0 ? d / r : 1.0, s2 = r > 0.0 ? 2.0 * j12 / r : 0.0;
    double l1, l2;
    if (p.ced) {
        l1 = p.alpha;
        l2 = r > 0.0 ? p.alpha + (1.0 - p.alpha) * exp(-p.C / (r * r)) : p.alpha;
    } else {
        l2 = 1.0;
        if (mu1 > 0.0) {
            const double q = mu1 / (p.lambda * p.lambda), q2 = q * q;
            l1 = 1.0 - exp(-3.31488 / (q2 * q2));
        } else {
            l1 = 1.0;
        }
    }
    const double m = 0.5 * (l1 + l2), h = 0.5 * (l1 - l2);
    D11 = m + h * c2;
    D22 = m - h * c2;
    D12 = h * s2;
}

// The tile of tensor_tile_fill (pdeip_tv.hpp) with the tensors recomputed from J in the one-pixel halo; in the TV-8 assembly's
// names dyy := D11, dxx := D22, dxy := D12 (x along the columns, y down the rows).  Positions across the frame's edge wrap as there;
// the weights that read them are zeroed.
__device__ __forceinline__ void st_tile_fill(TensorTile &T, const float *J11, const float *J12, const float *J22, const TensorRule &p, int i0,
                                             int j0, int nrows, int ncols)
{
    const int tid = threadIdx.y * TT_R + threadIdx.x;
    for (int e = tid; e < (TT_C + 2) * (TT_R + 2); e += TT_R * TT_C) {
        const int c = e / (TT_R + 2), r = e - c * (TT_R + 2);
        int ii = i0 - 1 + r, jj = j0 - 1 + c;
        if (ii > nrows || jj > ncols) continue; // beyond the wrap position: no output pixel reads it
        ii = ii < 0 ? nrows - 1 : (ii > nrows - 1 ? 0 : ii);
        jj = jj < 0 ? ncols - 1 : (jj > ncols - 1 ? 0 : jj);
        const size_t q = (size_t)jj * nrows + ii;
        diffusion_tensor((double)J11[q], (double)J12[q], (double)J22[q], p, T.dyy[c][r], T.dxx[c][r], T.dxy[c][r]);
    }
}

// w8[k] = (float)(tau w_k), k = W NW N NE E SE S SW, and TRACE = (float)(1 + tau sum w): the semi-implicit step
// (I - tau A(u^k)) u^{k+1} = u^k as PDEsolver8 takes it.  One plane per weight, whatever the number of channels.
// pad = 1: the planes are [(nrows + 2) x (ncols + 2)], the image's weights inside a one-pixel ring of TRACE = 1 and zero weights
// (the pixels on the image's edge write the ring next to them).
__global__ void __launch_bounds__(TT_R *TT_C)
k_st_weights(float *TRACE, float *w8, const float *J11, const float *J12, const float *J22, TensorRule p, double tau, int nrows, int ncols, int pad)
{
    __shared__ TensorTile T;
    const int i0 = blockIdx.x * TT_R, j0 = blockIdx.y * TT_C;
    st_tile_fill(T, J11, J12, J22, p, i0, j0, nrows, ncols);
    __syncthreads();
    const int i = i0 + threadIdx.x, j = j0 + threadIdx.y;
    if (i >= nrows || j >= ncols) return;
    const int ld = nrows + 2 * pad;
    const size_t n = (size_t)ld * (ncols + 2 * pad), pos = (size_t)(j + pad) * ld + (i + pad);
    double w[8];
    const double sum = tensor_weights8(T, threadIdx.y + 1, threadIdx.x + 1, j == 0, j == ncols - 1, i == 0, i == nrows - 1, w);
    TRACE[pos] = (float)(1.0 + tau * sum);
#pragma unroll
    for (int k = 0; k < 8; ++k) w8[(size_t)k * n + pos] = (float)(tau * w[k]);
    if (pad) {
        const int di = i == 0 ? -1 : (i == nrows - 1 ? 1 : 0), dj = j == 0 ? -1 : (j == ncols - 1 ? 1 : 0);
        auto ring = [&](int a, int b) {
            const size_t q = (size_t)(j + pad + b) * ld + (i + pad + a);
            TRACE[q] = 1.0f;
#pragma unroll
            for (int k = 0; k < 8; ++k) w8[(size_t)k * n + q] = 0.0f;
        };
        if (di) ring(di, 0);
        if (dj) ring(0, dj);
        if (di && dj) ring(di, dj);
    }
}

// out (and out2, unless null) [(nrows + 2) x (ncols + 2) x frames] = in [nrows x ncols x frames] inside a one-pixel ring of its
// nearest pixels.  PDEsolver8 relaxes the interior of a plane and copies the neighbours into its outer ring after every sweep:
// inside this ring every pixel of the image is relaxed, and the ring is the solver's.  Grid: pixel_grid(nrows + 2, ncols + 2, frames).
__global__ void k_st_pad(float *out, float *out2, const float *in, int nrows, int ncols)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y, pr = nrows + 2, pc = ncols + 2;
    if (i >= pr) return;
    const float v = in[(size_t)blockIdx.z * nrows * ncols + (size_t)clampi(j - 1, ncols - 1) * nrows + clampi(i - 1, nrows - 1)];
    const size_t q = (size_t)blockIdx.z * pr * pc + (size_t)j * pr + i;
    out[q] = v;
    if (out2 != nullptr) out2[q] = v;
}

// The inverse: out [nrows x ncols x frames] = the inside of in.  Grid: pixel_grid(nrows, ncols, frames).
__global__ void k_st_crop(float *out, const float *in, int nrows, int ncols)
{
    PDEIP_PIXEL_INDEX();
    const int pr = nrows + 2;
    out[(size_t)blockIdx.z * nrows * ncols + pos] = in[(size_t)blockIdx.z * pr * (ncols + 2) + (size_t)(j + 1) * pr + (i + 1)];
}

} // namespace st
} // namespace pdeip
