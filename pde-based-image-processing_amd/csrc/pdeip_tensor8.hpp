// pdeip_tensor8.hpp -- the 9-point discretisation of div(D grad u) from a per-pixel tensor D = [dxx dxy; dxy dyy]: the tile of
// tensors a workgroup keeps in LDS and the eight weights assembled from it.  Shared by the kernels of pdeip_tv.hpp (TVdenoise8's
// ADdiffWeights, the AD flow driver) and pdeip_stensor.hpp (EED / CED), so that all of them have one assembly with one set of bits.
#pragma once
#include <hip/hip_runtime.h>

namespace pdeip {

// A workgroup of 64 x 4 threads owns 64 rows x 4 columns and evaluates the diffusion tensor ONCE for its 66 x 6 neighbourhood into
// LDS -- circshift wrap-around at the frame edges as the drivers have it -- instead of nine times per output pixel.
constexpr int TT_R = 64, TT_C = 4;
struct TensorTile {
    double dyy[TT_C + 2][TT_R + 2], dxx[TT_C + 2][TT_R + 2], dxy[TT_C + 2][TT_R + 2];
};

// The eight weights at tile position (c, r) from the tensors of the pixel and its neighbours, in the order W NW N NE E SE S SW, a
// weight across the frame's edge zeroed (c0 / cE: first / last column, r0 / rE: first / last row), and their sum, left to right.
__device__ __forceinline__ double tensor_weights8(const TensorTile &T, int c, int r, bool c0, bool cE, bool r0, bool rE, double w[8])
{
    const double dyy = T.dyy[c][r], dxx = T.dxx[c][r], dxy = T.dxy[c][r];
    w[0] = c0 ? 0.0 : 0.5 * (dyy + T.dyy[c - 1][r]);
    w[1] = (c0 || r0) ? 0.0 : 0.25 * (dxy + T.dxy[c - 1][r - 1]);
    w[2] = r0 ? 0.0 : 0.5 * (dxx + T.dxx[c][r - 1]);
    w[3] = (cE || r0) ? 0.0 : -0.25 * (dxy + T.dxy[c + 1][r - 1]);
    w[4] = cE ? 0.0 : 0.5 * (dyy + T.dyy[c + 1][r]);
    w[5] = (cE || rE) ? 0.0 : 0.25 * (dxy + T.dxy[c + 1][r + 1]);
    w[6] = rE ? 0.0 : 0.5 * (dxx + T.dxx[c][r + 1]);
    w[7] = (rE || c0) ? 0.0 : -0.25 * (dxy + T.dxy[c - 1][r + 1]);
    double sum = w[0] + w[1]; // wW+wNW+wN+wNE+wE+wSE+wS+wSW, left to right
    sum = sum + w[2];
    sum = sum + w[3];
    sum = sum + w[4];
    sum = sum + w[5];
    sum = sum + w[6];
    sum = sum + w[7];
    return sum;
}

} // namespace pdeip
