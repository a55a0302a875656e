// pdeip_sparse_plan.hpp -- what the sparse driver's calls decide on the host before their HIP calls (DispSegmentationSparse.m:42-79,
// 226): the argument checks of pdeip_nanmedfilt2 and pdeip_sparse_pyramid, the scale sizes (the rule of pdeip_seeds_plan.hpp), the
// layout of the pyramid and of the builder's two temporaries, and the constants in which the sparse stages differ from the dense
// ones.  Plain C++ (no HIP, no library state), so that tools/sparse_plan_check.cpp can run it under the host sanitizers;
// csrc/pdeip_sparse.hip and csrc/pdeip_segmentation.hip are its other users.
#pragma once
#include "pdeip_seeds_plan.hpp"

#include <climits>
#include <cstddef>

namespace pdeip {
namespace sparse {

constexpr double GAMMA0 = 0.005;    // generateSeeds()'s starting gamma in the sparse driver (:226); seeds::GAMMA0 in the dense one
constexpr int MAX_GRID_YZ = 65535;  // columns are on blockIdx.y and frames on blockIdx.z of the per-pixel geometry

// NULL when pdeip_nanmedfilt2(_dev) accepts the arguments, else what is wrong with them, formatted into buf.  *unsupported is set
// when the refusal is the launch geometry's (more than 65535 columns or frames) and not the contract's.
inline const char *check_filter(char *buf, size_t cap, const void *A, const void *out, int nrows, int ncols, int nframes, bool *unsupported)
{
    *unsupported = false;
    if (A == nullptr) return std::snprintf(buf, cap, "argument 'A' is NULL"), buf;
    if (out == nullptr) return std::snprintf(buf, cap, "argument 'out' is NULL"), buf;
    if (nrows < 1 || ncols < 1) return std::snprintf(buf, cap, "the plane must be at least 1x1 (got %dx%d)", nrows, ncols), buf;
    if (nframes < 1) return std::snprintf(buf, cap, "number of frames must be >= 1 (got %d)", nframes), buf;
    if ((long long)nrows * (long long)ncols > (long long)INT_MAX) return std::snprintf(buf, cap, "a plane of more than INT_MAX pixels"), buf;
    if (A == out) return std::snprintf(buf, cap, "out must not alias A"), buf;
    if (ncols > MAX_GRID_YZ || nframes > MAX_GRID_YZ) {
        *unsupported = true;
        return std::snprintf(buf, cap, "more than %d columns or frames (got %d, %d)", MAX_GRID_YZ, ncols, nframes), buf;
    }
    return nullptr;
}

// pdeip_sparse_pyramid (D and the outputs are checked by the caller: out may be NULL).
inline const char *check_pyramid(char *buf, size_t cap, int nrows, int ncols, double scl_factor, double pyr_scl, int scales_cap)
{
    if (nrows < 3 || ncols < 3) return std::snprintf(buf, cap, "D must be at least 3x3 (got %dx%d)", nrows, ncols), buf;
    if ((long long)nrows * (long long)ncols > (long long)INT_MAX) return std::snprintf(buf, cap, "a plane of more than INT_MAX pixels"), buf;
    if (!(scl_factor > 0.0 && scl_factor < 1.0)) return std::snprintf(buf, cap, "scl_factor must lie in (0, 1) (got %g)", scl_factor), buf;
    if (!(pyr_scl > 0.0) || !std::isfinite(pyr_scl)) return std::snprintf(buf, cap, "pyr_scl must be finite and > 0 (got %g)", pyr_scl), buf;
    if (scales_cap < 1) return std::snprintf(buf, cap, "scales_cap must be >= 1 (got %d)", scales_cap), buf;
    return nullptr;
}

inline size_t pad4(size_t n) { return (n + 3) & ~(size_t)3; }
inline size_t pixels(const seeds::Size &q) { return (size_t)q.r * (size_t)q.c; }

// Where the planes live, in floats from the start of one buffer: the K scales packed in scale order (every offset a multiple of 4
// floats), then the builder's temporaries: t1 holds nanmed(P_k), as large as scale 1; t2 its resize, as large as scale 2.
struct Layout {
    std::vector<size_t> scale; // offset of P_k
    size_t t1, t2, total;
    int launches;              // 3K - 2: P_1 = nanmed(D); per further scale nanmed, resize, nanmed
};
inline Layout layout(const std::vector<seeds::Size> &sz)
{
    Layout L;
    size_t at = 0;
    for (const seeds::Size &q : sz) {
        L.scale.push_back(at);
        at += pad4(pixels(q));
    }
    L.t1 = at;
    at += sz.size() > 1 ? pad4(pixels(sz[0])) : 0;
    L.t2 = at;
    at += sz.size() > 1 ? pad4(pixels(sz[1])) : 0;
    L.total = at;
    L.launches = 3 * (int)sz.size() - 2;
    return L;
}

// Floats of pdeip_sparse_pyramid's `out`: the planes packed without padding, in scale order.
inline size_t packed_floats(const std::vector<seeds::Size> &sz)
{
    size_t n = 0;
    for (const seeds::Size &q : sz) n += pixels(q);
    return n;
}

// ---- the constants of the sparse stages: what a NaN member or a NULL struct resolves to ----
inline seeds::Prm seeds_defaults() { return seeds::Prm{100.0, 0.5, 1000.0f}; } // dist_cap, mincov_gate, nan_fill
inline seeds::Prm dense_seeds_defaults() { return seeds::resolve(nullptr, nullptr, nullptr); }
inline seeds::Prm resolve(seeds::Prm p, const double *dist_cap, const double *nan_fill, const double *mincov_gate)
{
    if (dist_cap && !std::isnan(*dist_cap)) p.dist_cap = *dist_cap;
    if (nan_fill && !std::isnan(*nan_fill)) p.nan_fill = (float)*nan_fill;
    if (mincov_gate && !std::isnan(*mincov_gate)) p.mincov_gate = *mincov_gate;
    return p;
}

// DispSegmentationSparse.m:42-56
inline seeds::DriverPrm driver_defaults() { return seeds::DriverPrm{0.002, 0.75, 0.55, 0.55, 0.1, 0.7, 2, 15, 10}; }

} // namespace sparse
} // namespace pdeip
