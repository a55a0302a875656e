// pdeip_sym_warp.hpp -- interp2(X, Y, U, X+Uq, Y) at one pixel: the warp of the symmetric stereo driver (k_sym_warp_flow,
// csrc/pdeip_sym.hpp) and of the disparity cross-check (k_disp_crosscheck, csrc/pdeip_crosscheck.hpp), which are the same value bit
// for bit because they are this one function.
#pragma once
#include <hip/hip_runtime.h>

namespace pdeip {

// The query rows are the grid rows, so only x is interpolated: linear, NaN outside 1 <= xq <= ncols (interp2's documented default).
// uq is Uq at (i, j); a tap with weight 0 still propagates its NaN.  Needs ncols >= 2.
__device__ __forceinline__ double sym_warp_at(const float *U, float uq, int i, int j, int nrows, int ncols)
{
    const double xq = (double)(j + 1) + (double)uq;
    if (!(xq >= 1.0 && xq <= (double)ncols)) return __longlong_as_double(0x7ff8000000000000LL); // also a NaN query
    double j0 = floor(xq);
    if (j0 > (double)(ncols - 1)) j0 = (double)(ncols - 1); // xq == ncols: the last column itself (s = 1)
    const double s = xq - j0;
    const int c0 = (int)j0 - 1, c1 = min(c0 + 1, ncols - 1);
    return (double)U[(size_t)c0 * nrows + i] * (1.0 - s) + (double)U[(size_t)c1 * nrows + i] * s;
}

} // namespace pdeip
