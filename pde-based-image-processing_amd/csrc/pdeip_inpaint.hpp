// pdeip_inpaint.hpp -- the stages of total-variation inpainting of a sparse map (NaN = no estimate) as device kernels: the NaN-aware
// resize of the pyramid, the starting fill of the coarsest scale, the assembly of TRACE / B / the lagged-diffusivity weights with an
// optional guide image, and the merge that hands the known pixels their own bits back.  The solver between assembly and merge is the
// library's own PDEsolver4 (pdeip_pde_sor4_dev / pdeip_pde_alr4_dev), whose NaN-TRACE branch fills a hole by diffusion alone.
//
// These are this library's own definitions (include/pdeip.h); tests/inpaint_ref.py is the numpy statement the tests compare with,
// bit for bit.  All single arithmetic is FMA-free (-ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>

#include "pdeip_pointwise.hpp"
#include "pdeip_pyr.hpp"

namespace pdeip {
namespace inpaint {

constexpr int FILL_BLOCK = 256; // columns a workgroup of k_inpaint_meanfill sums at once
constexpr int FLAT_BLOCK = 256;

// pyramid.resize of where(known, D, 0) and of the 0/1 plane `known`, both in double, one walk of k_pyr_resize's tap lists with both
// sums in its order; out = (float)(num / den) where den >= cover, NaN elsewhere.
__global__ void k_nan_resize(float *out, const float *in, PyrAxis R, PyrAxis C, int nrows_in, int ncols_in, int nrows, int ncols, double cover)
{
    PDEIP_PIXEL_INDEX();
    const float *src = in + (size_t)blockIdx.z * nrows_in * ncols_in;
    const double xr = ((double)i + 0.5) / R.scale - 0.5, xc = ((double)j + 0.5) / C.scale - 0.5;
    const int fr = (int)floor(xr - R.width), fc = (int)floor(xc - C.width);
    double rw[PYR_TMAX], rtot = 0.0, ctot = 0.0;
    for (int k = 0; k < R.T; ++k) {
        rw[k] = pyr_weight(R, xr, fr + k);
        rtot = k ? rtot + rw[k] : rw[k];
    }
    for (int k = 0; k < C.T; ++k) {
        const double w = pyr_weight(C, xc, fc + k);
        ctot = k ? ctot + w : w;
    }
    double num = 0.0, den = 0.0;
    for (int kc = 0; kc < C.T; ++kc) {
        const float *col = src + (size_t)min(max(fc + kc, 0), ncols_in - 1) * nrows_in;
        double tn = 0.0, td = 0.0;
        for (int kr = 0; kr < R.T; ++kr) {
            const float v = col[min(max(fr + kr, 0), nrows_in - 1)];
            const bool known = v == v;
            const double w = rw[kr] / rtot;
            const double vn = w * (known ? (double)v : 0.0), vd = w * (known ? 1.0 : 0.0);
            tn = kr ? tn + vn : vn;
            td = kr ? td + vd : vd;
        }
        const double w = pyr_weight(C, xc, fc + kc) / ctot;
        const double vn = w * tn, vd = w * td;
        num = kc ? num + vn : vn;
        den = kc ? den + vd : vd;
    }
    out[(size_t)blockIdx.z * nrows * ncols + pos] = den >= cover ? (float)(num / den) : __int_as_float(0x7fc00000);
}

// One workgroup per frame.  A thread sums one column's known values top to bottom in double; thread 0 adds the column sums left to
// right (FILL_BLOCK columns per round, the rounds in order, so the whole sum runs left to right); mean = (float)(sum / count), 0 for a
// frame without a number; then holes take the mean and known pixels keep their bits.
__global__ void __launch_bounds__(FILL_BLOCK) k_inpaint_meanfill(float *out, const float *D, int nrows, int ncols)
{
    __shared__ double s_sum[FILL_BLOCK];
    __shared__ unsigned int s_cnt[FILL_BLOCK];
    __shared__ float s_mean;
    const size_t n = (size_t)nrows * ncols;
    const float *P = D + (size_t)blockIdx.x * n;
    float *O = out + (size_t)blockIdx.x * n;
    const int t = threadIdx.x;
    double total = 0.0;          // thread 0's
    unsigned long long count = 0; // thread 0's
    for (int j0 = 0; j0 < ncols; j0 += FILL_BLOCK) {
        const int j = j0 + t;
        double acc = 0.0;
        unsigned int cnt = 0;
        if (j < ncols) {
            const float *col = P + (size_t)j * nrows;
            for (int i = 0; i < nrows; ++i) {
                const float v = col[i];
                const bool known = v == v;
                acc = acc + (known ? (double)v : 0.0);
                cnt += known ? 1u : 0u;
            }
        }
        s_sum[t] = acc;
        s_cnt[t] = cnt;
        __syncthreads();
        if (t == 0) {
            const int m = min(FILL_BLOCK, ncols - j0);
            for (int k = 0; k < m; ++k) {
                total = total + s_sum[k];
                count += s_cnt[k];
            }
        }
        __syncthreads();
    }
    if (t == 0) s_mean = count ? (float)(total / (double)count) : 0.0f;
    __syncthreads();
    const float mean = s_mean;
    for (size_t p = t; p < n; p += FILL_BLOCK) {
        const float v = P[p];
        O[p] = v == v ? v : mean;
    }
}

// k_tv4_assemble (pdeip_tv.hpp) with two changes: the maximum over the frames runs over X's frames and then over the guide's planes
// times guide_scale (rounded to single per value), and a pixel whose D is NaN gets TRACE = NaN, B = 0 -- the solvers' "no data here".
// The same expressions in the same order otherwise, so without holes and without a guide the bits are k_tv4_assemble's.
__global__ void k_tv4_inpaint_assemble(float *TRACE, float *B, float *aW, float *aN, float *aE, float *aS, const float *X, const float *D,
                                       const float *guide, int guide_channels, float guide_scale, float alpha, int nrows, int ncols, int nframes)
{
    PDEIP_PIXEL_INDEX();
    const size_t n = (size_t)nrows * ncols;
    auto wrap_i = [&](int v) { return v < 0 ? nrows - 1 : (v > nrows - 1 ? 0 : v); };
    auto wrap_j = [&](int v) { return v < 0 ? ncols - 1 : (v > ncols - 1 ? 0 : v); };
    float m[4] = {0.0f, 0.0f, 0.0f, 0.0f}; // W, E, N, S
    for (int f = 0; f < nframes + guide_channels; ++f) {
        const bool g = f >= nframes;
        const float *P = g ? guide + (size_t)(f - nframes) * n : X + (size_t)f * n;
        auto at = [&](int ii, int jj) {
            const float v = P[(size_t)jj * nrows + ii];
            return g ? guide_scale * v : v;
        };
        auto ver = [&](int ii, int jj) { return 0.25f * at(max(ii - 1, 0), jj) - 0.25f * at(min(ii + 1, nrows - 1), jj); };
        auto hor = [&](int ii, int jj) { return 0.25f * at(ii, max(jj - 1, 0)) - 0.25f * at(ii, min(jj + 1, ncols - 1)); };
        const float c = at(i, j);
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const int ii = d == 2 ? wrap_i(i - 1) : (d == 3 ? wrap_i(i + 1) : i), jj = d == 0 ? wrap_j(j - 1) : (d == 1 ? wrap_j(j + 1) : j);
            const float a = at(ii, jj) - c;
            const float b = d < 2 ? ver(i, j) + ver(ii, jj) : hor(i, j) + hor(ii, jj);
            const float v = a * a + b * b;
            m[d] = f == 0 ? v : fmaxf(m[d], v);
        }
    }
    float w[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) w[d] = 1.0f / sqrtf(m[d] + 0.00001f);
    if (j == 0) w[0] = 0.0f;
    if (j == ncols - 1) w[1] = 0.0f;
    if (i == 0) w[2] = 0.0f;
    if (i == nrows - 1) w[3] = 0.0f;
    const float tot = ((w[0] + w[2]) + w[1]) + w[3]; // wW+wN+wE+wS
    const float atot = alpha * tot;
    for (int f = 0; f < nframes; ++f) {
        const size_t p = (size_t)f * n + pos;
        const float d = D[p];
        if (d == d) {
            const float diff = X[p] - d;
            const float psi = 1.0f / sqrtf(diff * diff + 2.220446049250313e-16f);
            TRACE[p] = psi + atot;
            B[p] = psi * d;
        } else { // a hole: D's NaN enters no arithmetic
            TRACE[p] = __int_as_float(0x7fc00000);
            B[p] = 0.0f;
        }
        aW[p] = alpha * w[0];
        aE[p] = alpha * w[1];
        aN[p] = alpha * w[2];
        aS[p] = alpha * w[3];
    }
}

// out = D where D is a number (its own bits), X elsewhere; filled = 1 on holes, 0 elsewhere.  Either output may be null.
__global__ void __launch_bounds__(FLAT_BLOCK) k_inpaint_merge(float *out, float *filled, const float *X, const float *D, size_t n)
{
    const size_t stride = (size_t)gridDim.x * FLAT_BLOCK;
    for (size_t p = (size_t)blockIdx.x * FLAT_BLOCK + threadIdx.x; p < n; p += stride) {
        const float d = D[p];
        const bool known = d == d;
        if (out) out[p] = known ? d : X[p];
        if (filled) filled[p] = known ? 0.0f : 1.0f;
    }
}

} // namespace inpaint
} // namespace pdeip
