// pdeip_sparse.hpp -- k_nanmedian3: nanmedfilt2() of matlab/segmentation/DispSegmentationSparse.m:679-685, that is
// colfilt(D, [3 3], 'sliding', @nanmedian): the NaN-ignoring median of the 3x3 window, positions outside the plane holding the VALUE 0
// (colfilt's zero padding).  The contract is in include/pdeip.h; tests/sparse_ref.py restates it.
//
// One pixel per lane in the project's per-pixel geometry (256 lanes down the contiguous row index, columns on blockIdx.y, frames on
// blockIdx.z).  The nine values are sorted completely by a 25-exchange network of cswap (NaN above +Inf), after which the n numbers
// are the first n slots and n is the count of v == v.  The median is ((double)v[(n-1)/2] + (double)v[n/2]) * 0.5 rounded to single:
// for odd n both slots are the same value and the expression returns it unchanged (a + a and the halving are exact in double, for
// infinities and both zeros too), for even n it is the correctly rounded mean of the two middle values.  The two slots are picked
// by compile-time-indexed selects, so the array stays in registers.
#pragma once
#include "pdeip_ctx.hpp"
#include "pdeip_cswap.hpp"
#include "pdeip_pointwise.hpp"

namespace pdeip {

__global__ void __launch_bounds__(256) k_nanmedian3(float *__restrict__ out, const float *__restrict__ A, int nrows, int ncols)
{
    PDEIP_PIXEL_INDEX();
    const size_t frame = (size_t)blockIdx.z * ((size_t)nrows * (size_t)ncols);
    A += frame;
    out += frame;
    float v[9];
#pragma unroll
    for (int dj = -1; dj <= 1; ++dj)
#pragma unroll
        for (int di = -1; di <= 1; ++di) {
            const int ii = i + di, jj = j + dj;
            const bool inside = ii >= 0 && ii < nrows && jj >= 0 && jj < ncols;
            v[(dj + 1) * 3 + di + 1] = inside ? A[(size_t)jj * nrows + ii] : 0.0f;
        }
    // 25-exchange sorting network of nine inputs
    cswap(v[0], v[3]); cswap(v[1], v[7]); cswap(v[2], v[5]); cswap(v[4], v[8]);
    cswap(v[0], v[7]); cswap(v[2], v[4]); cswap(v[3], v[8]); cswap(v[5], v[6]);
    cswap(v[0], v[2]); cswap(v[1], v[3]); cswap(v[4], v[5]); cswap(v[7], v[8]);
    cswap(v[1], v[4]); cswap(v[3], v[6]); cswap(v[5], v[7]);
    cswap(v[0], v[1]); cswap(v[2], v[4]); cswap(v[3], v[5]); cswap(v[6], v[8]);
    cswap(v[2], v[3]); cswap(v[4], v[5]); cswap(v[6], v[7]);
    cswap(v[1], v[2]); cswap(v[3], v[4]); cswap(v[5], v[6]);
    int n = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) n += v[k] == v[k] ? 1 : 0;
    const int lo = (n - 1) >> 1, hi = n >> 1; // n == 0: lo = -1 matches no slot and the NaN below stays
    float a = __builtin_nanf(""), b = a;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        a = k == lo ? v[k] : a;
        b = k == hi ? v[k] : b;
    }
    out[pos] = (float)(((double)a + (double)b) * 0.5);
}

} // namespace pdeip
