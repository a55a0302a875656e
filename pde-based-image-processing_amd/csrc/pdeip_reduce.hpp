// pdeip_reduce.hpp -- the wave step of the library's fixed-order float64 sums (k_ransac_score's error sums, csrc/pdeip_ransac.hpp;
// the per-segment sums of csrc/pdeip_segmentation.hpp).  A sum is: the thread's value, this butterfly over the wave, the waves of the
// workgroup in ascending order through LDS, the tile partials in ascending tile order by one thread of a final pass.
#pragma once
#include <hip/hip_runtime.h>

namespace pdeip {

// The sum over the wave, partners FROM, FROM/2, .. 1 lanes apart (FROM = 32: the whole wave; k_ransac_score enters at 4, its first
// three steps being the paired ones): every lane ends with the same tree of additions (IEEE addition commutes), so equal inputs
// give equal bits wherever they stand.
template <int FROM = 32>
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int d = FROM; d >= 1; d >>= 1) v = v + __shfl_xor(v, d, 64);
    return v;
}

} // namespace pdeip
