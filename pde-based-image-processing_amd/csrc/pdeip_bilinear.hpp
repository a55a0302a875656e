// pdeip_bilinear.hpp -- the bilinear sample at a 1-based point (xq, yq) of a column-major plane: the sampler of the flow cross-check
// (k_flow_crosscheck, csrc/pdeip_crosscheck.hpp) and of the frame interpolation (k_flow_splat, k_interp_blend, csrc/pdeip_interp.hpp),
// which give the same value bit for bit because they are these two functions.
#pragma once
#include <hip/hip_runtime.h>

namespace pdeip {

// The taps of a sample: the 0-based rows r0, r1 and columns c0, c1 and the weights s (along x, columns) and t (along y, rows).
struct BilinearTaps {
    int r0, r1, c0, c1;
    double s, t;
};

// In range iff 1 <= xq <= ncols and 1 <= yq <= nrows (a NaN query fails); then j0 = min(floor(xq), ncols-1), s = xq - j0, rows
// alike, the +1 taps clamped to the last column / row.  Needs nrows, ncols >= 2.
__device__ __forceinline__ bool bilinear_taps(double xq, double yq, int nrows, int ncols, BilinearTaps *T)
{
    if (!(xq >= 1.0 && xq <= (double)ncols && yq >= 1.0 && yq <= (double)nrows)) return false;
    double j0 = floor(xq), i0 = floor(yq);
    if (j0 > (double)(ncols - 1)) j0 = (double)(ncols - 1); // xq == ncols: the last column itself (s = 1)
    if (i0 > (double)(nrows - 1)) i0 = (double)(nrows - 1);
    T->s = xq - j0;
    T->t = yq - i0;
    T->c0 = (int)j0 - 1;
    T->c1 = min(T->c0 + 1, ncols - 1);
    T->r0 = (int)i0 - 1;
    T->r1 = min(T->r0 + 1, nrows - 1);
    return true;
}

// B(A) at the 0-based taps (r0, c0), (r0, c1), (r1, c0), (r1, c1): s along x (columns), t along y (rows), in exactly this order.
__device__ __forceinline__ double bilinear(const float *__restrict__ A, int nrows, int r0, int r1, int c0, int c1, double s, double t)
{
    const size_t a0 = (size_t)c0 * nrows, a1 = (size_t)c1 * nrows;
    const double top = (double)A[a0 + r0] * (1.0 - s) + (double)A[a1 + r0] * s;
    const double bot = (double)A[a0 + r1] * (1.0 - s) + (double)A[a1 + r1] * s;
    return top * (1.0 - t) + bot * t;
}

__device__ __forceinline__ double bilinear(const float *__restrict__ A, int nrows, const BilinearTaps &T)
{
    return bilinear(A, nrows, T.r0, T.r1, T.c0, T.c1, T.s, T.t);
}

} // namespace pdeip
