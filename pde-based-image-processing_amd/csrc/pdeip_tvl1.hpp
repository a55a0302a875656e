// pdeip_tvl1.hpp -- kernels of TV-L1 optical flow (Zach, Pock and Bischof; Chambolle and Pock's first-order primal-dual iteration on the
// linearised brightness constancy of one warp).  The recurrence is the contract of include/pdeip.h, float32 without contraction,
// restated by tests/tvl1_ref.py:
//
//   ub = (u + u) - u_prev, vb likewise;  q* = p* + sigma * grad(ub | vb)  [/ (1 + sigma huber)];  p*' = q* / max(1, |q|), |q| the JOINT
//   norm of the four;  a = u + tau * div(pu'), b = v + tau * div(pv');  (u', v') = (a, b) + c * (gx, gy), c the thresholding step of
//   rho = (rc + gx a) + gy b;  u_prev' = u, v_prev' = v
//
// grad is the forward difference (0 on the last row / column), div its negative adjoint (a missing north / west neighbour drops out).
// Every pixel of an iteration depends on the previous iterate alone, so nothing depends on the order of evaluation.
//
//   k_tvl1_rc     rc = ((W - I0) - gx U0) - gy V0, one thread per pixel, lanes running down a column.
//   k_tvl1_step   one iteration per launch, one thread per pixel, lanes running down a column, no barrier.  A thread computes the four
//                 p' of its own pixel and recomputes those of its north and of its west neighbour (the joint norm needs all four q of
//                 each): seven values of ub and of vb, three of each p -- the repeated loads hit L1 / L2.  Reads u, u_prev, v, v_prev,
//                 four p, rc, gx, gy (11 planes); writes u', v' and four p' (6 planes); u_prev' and v_prev' are the u and v it read.
//   k_tvl1_block<T>  T iterations per launch: a workgroup holds a TILE_R x TILE_C tile of u, v, ub, vb, the four p, rc, gx, gy (eleven
//                 planes) in LDS with a halo of T pixels on every side and iterates on all of it, two barriers per iteration.  A
//                 pixel's state after k iterations depends on nothing farther than k pixels away, so after T iterations everything T
//                 or more pixels inside the LDS region is exact; the rings nearer to a cut edge hold values that are never stored.
//                 The border rules hold at the IMAGE border only; halo pixels outside the image are never computed or read.  Reads 11
//                 planes and writes 8 per T iterations.  The same bits as the step.
//
// P == nullptr: the dual variables are zero, nothing is read.  Po == nullptr: the last launch of a call that does not hand its duals
// on.  Only scalar 4-byte loads and stores: a plane may start at any 4-byte offset.  u and u_prev may be the same plane (the start);
// no output may be an input.
#pragma once
#include <hip/hip_runtime.h>

namespace pdeip {
namespace tvl1 {

constexpr int BLOCK = 256;
// Rows (the contiguous direction) x columns of a blocked tile: k_tvpd_block's measured choice.
constexpr int TILE_R = 32, TILE_C = 16;

template <int T>
constexpr size_t block_lds_bytes() { return (size_t)11 * (TILE_R + 2 * T) * (TILE_C + 2 * T) * sizeof(float); }

// The call's constants, each formed once on the host in float32.
struct Consts {
    float sigma, tau;
    float tl;      // tau * lambda
    float hub_den; // 1 + sigma * huber
    int huber;     // 1: divide q by hub_den
};

// The four dual planes of a call: pxu, pyu, pxv, pyv, each nrows x ncols.
struct Duals {
    float *pxu, *pyu, *pxv, *pyv;
};
struct ConstDuals {
    const float *pxu, *pyu, *pxv, *pyv;
};

struct Dual4 {
    float xu, yu, xv, yv;
};

// p' of one pixel from ub, vb at the pixel (c), south (s) and east (e) of it (has_s / has_e: that neighbour exists) and its p.
__device__ __forceinline__ Dual4 dual(float ubc, float ubs, float ube, float vbc, float vbs, float vbe, bool has_s, bool has_e, const Dual4 &p,
                                      const Consts &c)
{
    const float gxu = has_s ? ubs - ubc : 0.0f, gyu = has_e ? ube - ubc : 0.0f;
    const float gxv = has_s ? vbs - vbc : 0.0f, gyv = has_e ? vbe - vbc : 0.0f;
    float qxu = p.xu + c.sigma * gxu, qyu = p.yu + c.sigma * gyu, qxv = p.xv + c.sigma * gxv, qyv = p.yv + c.sigma * gyv;
    if (c.huber) {
        qxu = qxu / c.hub_den;
        qyu = qyu / c.hub_den;
        qxv = qxv / c.hub_den;
        qyv = qyv / c.hub_den;
    }
    const float s = sqrtf((qxu * qxu + qyu * qyu) + (qxv * qxv + qyv * qyv));
    const float n = s > 1.0f ? s : 1.0f; // a NaN norm divides by 1
    return Dual4{qxu / n, qyu / n, qxv / n, qyv / n};
}

// (u', v') from a = u + tau div pu', b = v + tau div pv', the linearisation (rc, gx, gy); rc NaN: no data here.
__device__ __forceinline__ void primal(float a, float b, float rc, float gx, float gy, const Consts &c, float &un, float &vn)
{
    if (rc != rc) {
        un = a;
        vn = b;
        return;
    }
    const float g2 = gx * gx + gy * gy;
    const float rho = (rc + gx * a) + gy * b;
    const float t = c.tl * g2;
    // every comparison with a NaN is false: a NaN rho or g2 falls through to the last two branches
    const float k = rho > t ? -c.tl : (rho < -t ? c.tl : (g2 > 0.0f ? -rho / g2 : 0.0f));
    un = a + k * gx;
    vn = b + k * gy;
}

// Grid: (ceil(nrows / BLOCK), ncols).
__global__ __launch_bounds__(BLOCK) void k_tvl1_rc(const float *__restrict__ I0, const float *__restrict__ W, const float *__restrict__ GX,
                                                    const float *__restrict__ GY, const float *__restrict__ U0, const float *__restrict__ V0,
                                                    int nrows, int ncols, float *__restrict__ RC_)
{
    const int i = (int)blockIdx.x * BLOCK + (int)threadIdx.x, j = (int)blockIdx.y;
    if (i >= nrows) return;
    const size_t pos = (size_t)j * (size_t)nrows + (size_t)i;
    RC_[pos] = ((W[pos] - I0[pos]) - GX[pos] * U0[pos]) - GY[pos] * V0[pos];
}

// Grid: (ceil(nrows / BLOCK), ncols).  P.pxu == nullptr: zero duals; Po.pxu == nullptr: the duals are not stored.
__global__ __launch_bounds__(BLOCK) void k_tvl1_step(const float *U, const float *UP, const float *V, const float *VP, ConstDuals P,
                                                      const float *__restrict__ RC_, const float *__restrict__ GX, const float *__restrict__ GY,
                                                      int nrows, int ncols, Consts c, float *__restrict__ Uo, float *__restrict__ Vo, Duals Po)
{
    const int i = (int)blockIdx.x * BLOCK + (int)threadIdx.x, j = (int)blockIdx.y;
    if (i >= nrows) return;
    const size_t pos = (size_t)j * (size_t)nrows + (size_t)i;
    const size_t R = (size_t)nrows;
    const bool has_s = i + 1 < nrows, has_e = j + 1 < ncols, has_n = i > 0, has_w = j > 0, dual0 = P.pxu == nullptr;
    const auto ub = [&](size_t p) {
        const float u = U[p];
        return (u + u) - UP[p];
    };
    const auto vb = [&](size_t p) {
        const float v = V[p];
        return (v + v) - VP[p];
    };
    const auto duals_at = [&](size_t p) { return dual0 ? Dual4{0.0f, 0.0f, 0.0f, 0.0f} : Dual4{P.pxu[p], P.pyu[p], P.pxv[p], P.pyv[p]}; };
    const float u = U[pos], v = V[pos];
    const float ubc = (u + u) - UP[pos], vbc = (v + v) - VP[pos];
    const float ubs = has_s ? ub(pos + 1) : 0.0f, ube = has_e ? ub(pos + R) : 0.0f;
    const float vbs = has_s ? vb(pos + 1) : 0.0f, vbe = has_e ? vb(pos + R) : 0.0f;
    const Dual4 p = dual(ubc, ubs, ube, vbc, vbs, vbe, has_s, has_e, duals_at(pos), c);
    float du = p.xu, dv = p.xv;
    if (has_n) { // the north neighbour's south is this pixel
        const Dual4 pn = dual(ub(pos - 1), ubc, has_e ? ub(pos - 1 + R) : 0.0f, vb(pos - 1), vbc, has_e ? vb(pos - 1 + R) : 0.0f, true, has_e,
                              duals_at(pos - 1), c);
        du = p.xu - pn.xu;
        dv = p.xv - pn.xv;
    }
    float eu = p.yu, ev = p.yv;
    if (has_w) { // the west neighbour's east is this pixel
        const Dual4 pw = dual(ub(pos - R), has_s ? ub(pos - R + 1) : 0.0f, ubc, vb(pos - R), has_s ? vb(pos - R + 1) : 0.0f, vbc, has_s, true,
                              duals_at(pos - R), c);
        eu = p.yu - pw.yu;
        ev = p.yv - pw.yv;
    }
    const float a = u + c.tau * (du + eu), b = v + c.tau * (dv + ev);
    float un, vn;
    primal(a, b, RC_[pos], GX[pos], GY[pos], c, un, vn);
    Uo[pos] = un;
    Vo[pos] = vn;
    if (Po.pxu != nullptr) {
        Po.pxu[pos] = p.xu;
        Po.pyu[pos] = p.yu;
        Po.pxv[pos] = p.xv;
        Po.pyv[pos] = p.yv;
    }
}

// Grid: (ceil(nrows / TILE_R), ceil(ncols / TILE_C)); dynamic LDS: block_lds_bytes<T>().  UPo (with VPo) and Po.pxu may each be null.
template <int T>
__global__ __launch_bounds__(BLOCK) void k_tvl1_block(const float *U, const float *UP, const float *V, const float *VP, ConstDuals P,
                                                       const float *__restrict__ RC_, const float *__restrict__ GX, const float *__restrict__ GY,
                                                       int nrows, int ncols, Consts c, float *__restrict__ Uo, float *__restrict__ Vo,
                                                       float *__restrict__ UPo, float *__restrict__ VPo, Duals Po)
{
    constexpr int LR = TILE_R + 2 * T, LC = TILE_C + 2 * T, LN = LR * LC;
    extern __shared__ float tvl1_lds[];
    float *sU = tvl1_lds, *sV = sU + LN, *sBU = sV + LN, *sBV = sBU + LN, *sXU = sBV + LN, *sYU = sXU + LN, *sXV = sYU + LN, *sYV = sXV + LN;
    float *sRC = sYV + LN, *sGX = sRC + LN, *sGY = sGX + LN;
    const int t = (int)threadIdx.x;
    const int gi0 = (int)blockIdx.x * TILE_R - T, gj0 = (int)blockIdx.y * TILE_C - T; // the LDS region's first row and column
    const bool dual0 = P.pxu == nullptr;

    // a pixel of the region: local index k = lj * LR + li; it exists if it lies inside the image
    for (int k = t; k < LN; k += BLOCK) {
        const int lj = k / LR, li = k - lj * LR, gi = gi0 + li, gj = gj0 + lj;
        float u = 0.0f, v = 0.0f, bu = 0.0f, bv = 0.0f, xu = 0.0f, yu = 0.0f, xv = 0.0f, yv = 0.0f, rc = 0.0f, gx = 0.0f, gy = 0.0f;
        if (gi >= 0 && gi < nrows && gj >= 0 && gj < ncols) {
            const size_t p = (size_t)gj * (size_t)nrows + (size_t)gi;
            u = U[p];
            bu = (u + u) - UP[p];
            v = V[p];
            bv = (v + v) - VP[p];
            if (!dual0) {
                xu = P.pxu[p];
                yu = P.pyu[p];
                xv = P.pxv[p];
                yv = P.pyv[p];
            }
            rc = RC_[p];
            gx = GX[p];
            gy = GY[p];
        }
        sU[k] = u;
        sV[k] = v;
        sBU[k] = bu;
        sBV[k] = bv;
        sXU[k] = xu;
        sYU[k] = yu;
        sXV[k] = xv;
        sYV[k] = yv;
        sRC[k] = rc;
        sGX[k] = gx;
        sGY[k] = gy;
    }
    __syncthreads();

#pragma unroll 1
    for (int it = 0; it < T; it++) {
        // the dual step: a neighbour beyond the region's edge counts as missing, which spoils one more ring per iteration
        for (int k = t; k < LN; k += BLOCK) {
            const int lj = k / LR, li = k - lj * LR, gi = gi0 + li, gj = gj0 + lj;
            if (gi < 0 || gi >= nrows || gj < 0 || gj >= ncols) continue;
            const bool has_s = gi + 1 < nrows && li + 1 < LR, has_e = gj + 1 < ncols && lj + 1 < LC;
            const Dual4 p = dual(sBU[k], has_s ? sBU[k + 1] : 0.0f, has_e ? sBU[k + LR] : 0.0f, sBV[k], has_s ? sBV[k + 1] : 0.0f,
                                 has_e ? sBV[k + LR] : 0.0f, has_s, has_e, Dual4{sXU[k], sYU[k], sXV[k], sYV[k]}, c);
            sXU[k] = p.xu;
            sYU[k] = p.yu;
            sXV[k] = p.xv;
            sYV[k] = p.yv;
        }
        __syncthreads();
        // the primal step; the last one stores the tile
        for (int k = t; k < LN; k += BLOCK) {
            const int lj = k / LR, li = k - lj * LR, gi = gi0 + li, gj = gj0 + lj;
            if (gi < 0 || gi >= nrows || gj < 0 || gj >= ncols) continue;
            const bool has_n = gi > 0 && li > 0, has_w = gj > 0 && lj > 0;
            const float xu = sXU[k], yu = sYU[k], xv = sXV[k], yv = sYV[k], u = sU[k], v = sV[k];
            const float du = has_n ? xu - sXU[k - 1] : xu, dv = has_n ? xv - sXV[k - 1] : xv;
            const float eu = has_w ? yu - sYU[k - LR] : yu, ev = has_w ? yv - sYV[k - LR] : yv;
            float un, vn;
            primal(u + c.tau * (du + eu), v + c.tau * (dv + ev), sRC[k], sGX[k], sGY[k], c, un, vn);
            if (it < T - 1) {
                sU[k] = un;
                sV[k] = vn;
                sBU[k] = (un + un) - u;
                sBV[k] = (vn + vn) - v;
            } else if (li >= T && li < T + TILE_R && lj >= T && lj < T + TILE_C) {
                const size_t p = (size_t)gj * (size_t)nrows + (size_t)gi;
                Uo[p] = un;
                Vo[p] = vn;
                if (UPo != nullptr) {
                    UPo[p] = u;
                    VPo[p] = v;
                }
                if (Po.pxu != nullptr) {
                    Po.pxu[p] = xu;
                    Po.pyu[p] = yu;
                    Po.pxv[p] = xv;
                    Po.pyv[p] = yv;
                }
            }
        }
        __syncthreads();
    }
}

} // namespace tvl1
} // namespace pdeip
