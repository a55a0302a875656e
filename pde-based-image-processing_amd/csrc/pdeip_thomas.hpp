// pdeip_thomas.hpp -- the AOS line solve shared by the level-set step (pdeip_levelset.hpp), the Chan-Vese step (pdeip_cv.hpp)
// and Diffusion4_v10 (pdeip_diffusion.hpp): one lane per line, the Thomas recurrence serial inside the lane so that every
// operation keeps the reference's order.  (The zebra and lex line relaxations of pdeip_alr.hpp are a different design.)
//
// The coefficients a, b, c, d of CH consecutive elements are computed before the chain runs through them, so only b - cp*a,
// the reciprocal and the two multiplies sit on the dependency chain.  cp/dp live in a global scratch plane laid out so that
// the 64 lanes of a wave touch 64 consecutive floats at every step (Line, below); a line may have any length >= 2.
// -ffp-contract=off (build.py) keeps every product and sum separate.
#pragma once
#include <hip/hip_runtime.h>

namespace pdeip {
namespace thomas {

constexpr int CH = 8;     // elements whose coefficients are fetched ahead of the chain
constexpr int BLOCK = 64; // one wave per block: the few lines of a frame spread over as many CUs as possible

struct Coef {
    float a, b, c, d;
};

// Forward sweep of a line of n >= 2 elements: cp/dp of element k < n-1 go to sbase + k*sstride; returns x[n-1].
// coef_at(k) gives Coef of element k; it is called with min(k0 + u, n - 2) inside a chunk (the clamped tail of the last chunk
// is fetched and not used) and with 0 and n - 1 outside.
// The operation order is fixed here: cp*a and dp*a, the factors this way round.  Diffusion4_v10.m's TDMA writes a*cp and a*dp;
// IEEE multiplication commutes, so every value is the same, and only where both factors are NaN may the hardware hand on the
// other one's payload.  No check tells NaN payloads apart.
template <class CoefAt>
__device__ __forceinline__ float forward(CoefAt coef_at, float *__restrict__ cp, float *__restrict__ dp, size_t sbase,
                                         size_t sstride, int n)
{
    const Coef c0 = coef_at(0);
    float cpv = c0.c / c0.b;
    float dpv = c0.d / c0.b;
    cp[sbase] = cpv;
    dp[sbase] = dpv;
    for (int k0 = 1; k0 <= n - 2; k0 += CH) {
        Coef c[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) c[u] = coef_at(min(k0 + u, n - 2));
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int k = k0 + u;
            if (k <= n - 2) {
                const float div = 1.0f / (c[u].b - cpv * c[u].a);
                cpv = c[u].c * div;
                dpv = (c[u].d - dpv * c[u].a) * div;
                cp[sbase + (size_t)k * sstride] = cpv;
                dp[sbase + (size_t)k * sstride] = dpv;
            }
        }
    }
    const Coef cl = coef_at(n - 1);
    return (cl.d - dpv * cl.a) / (cl.b - cpv * cl.a); // the last element divides
}

// Plain back-substitution after forward(): x[n-1] = xlast, x[k] = dp[k] - cp[k]*x[k+1], CH elements of cp/dp fetched ahead of
// the chain.  store(k, x) is called for k = n-1 ... 0.
template <class Store>
__device__ __forceinline__ void back_plain(const float *__restrict__ cp, const float *__restrict__ dp, size_t sbase, size_t sstride,
                                           int n, float xlast, Store store)
{
    float x1 = xlast;
    store(n - 1, x1);
    for (int k0 = n - 2; k0 >= 0; k0 -= CH) {
        float cpk[CH], dpk[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int k = max(k0 - u, 0);
            cpk[u] = cp[sbase + (size_t)k * sstride];
            dpk[u] = dp[sbase + (size_t)k * sstride];
        }
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int k = k0 - u;
            if (k >= 0) {
                x1 = dpk[u] - cpk[u] * x1;
                store(k, x1);
            }
        }
    }
}

// Where a line lies: element k of the line at base + k*stride of a frame stack [nrows x ncols x frames] (column-major, frame
// offset fo), its cp/dp at sbase + k*sstride of a scratch plane of the same size.
struct Line {
    size_t base, stride, sbase, sstride;
    int n;
};
// Row i: strided by nrows, so the 64 rows of a wave are 64 consecutive floats at every step as they are; the scratch shares
// the image layout.
__device__ __forceinline__ Line row_line(size_t fo, int i, int nrows, int ncols)
{
    return Line{fo + i, (size_t)nrows, fo + i, (size_t)nrows, ncols};
}
// Column j: contiguous, so the 64 columns of a wave are nrows apart in the image; the scratch is kept transposed (element i of
// column j at i*ncols + j) so that at least the scratch traffic of a wave is one contiguous run per step.
__device__ __forceinline__ Line col_line(size_t fo, int j, int nrows, int ncols)
{
    return Line{fo + (size_t)j * nrows, 1, fo + j, (size_t)ncols, nrows};
}

// Both line kinds in one grid, for solves that do not read each other.  Blocks [0, row_blocks) hold the row lanes, the rest the
// column lanes: rows first, because at landscape shapes they are the longer chains and should start first.
enum Kind { ROW, COL, NONE };
struct Lane {
    Kind kind; // NONE: past the last row or column
    int idx;   // row i or column j
};
__device__ __forceinline__ Lane lane_of(int block, int row_blocks, int nrows, int ncols)
{
    if (block < row_blocks) {
        const int i = block * BLOCK + (int)threadIdx.x;
        return Lane{i < nrows ? ROW : NONE, i};
    }
    const int j = (block - row_blocks) * BLOCK + (int)threadIdx.x;
    return Lane{j < ncols ? COL : NONE, j};
}

// ---- host ----
inline int line_blocks(int nlines) { return (nlines + BLOCK - 1) / BLOCK; }
// Grid of a kernel that dispatches with lane_of(blockIdx.x, line_blocks(nrows), ...), blockIdx.y = frame.
inline dim3 lines_grid(int nrows, int ncols, int frames)
{
    return dim3((unsigned)(line_blocks(nrows) + line_blocks(ncols)), (unsigned)frames);
}
// The planes of such a kernel, p floats each: the column and row solutions and the column and row cp/dp.
struct Planes {
    float *xc, *xr, *cpc, *dpc, *cpr, *dpr;
};
inline Planes carve_planes(float *ws, size_t p) { return Planes{ws, ws + p, ws + 2 * p, ws + 3 * p, ws + 4 * p, ws + 5 * p}; }

} // namespace thomas
} // namespace pdeip
