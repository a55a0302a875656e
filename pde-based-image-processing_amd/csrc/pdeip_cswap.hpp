// pdeip_cswap.hpp -- the compare-exchange of the median kernels (k_median3_sum in pdeip_flow.hpp, k_nanmedian3 in pdeip_sparse.hpp).
// The order is that of an ascending sort with NaN as the largest value (above +Inf), as MATLAB's sort and numpy's place it.
// (fminf / fmaxf would drop a NaN and duplicate its partner.)  -0 and +0 compare equal and are not exchanged.
#pragma once
#include <hip/hip_runtime.h>

namespace pdeip {

__device__ __forceinline__ void cswap(float &a, float &b)
{
    const bool exchange = (a > b) || (a != a); // a NaN in the low slot moves up; two NaN trade places, which changes nothing
    const float lo = exchange ? b : a, hi = exchange ? a : b;
    a = lo;
    b = hi;
}

} // namespace pdeip
