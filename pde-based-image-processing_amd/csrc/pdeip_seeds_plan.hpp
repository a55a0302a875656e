// pdeip_seeds_plan.hpp -- what generateSeeds() and the dense driver decide on the host before and between their HIP calls: the
// argument checks, the scale sizes, the visit order and the per-iteration RANSAC schedule (DispSegmentation.m:56, 271-323).  Plain
// C++ (no HIP, no library state), so that tools/seeds_plan_check.cpp can run it under the host sanitizers;
// csrc/pdeip_segmentation.hip is its only other user.
#pragma once
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

namespace pdeip {
namespace seeds {

constexpr int EMPTY_BELOW = 20;     // numel(Xs) < 20 marks the seed empty (:332)
constexpr int RITER_FIRST = 2000;   // hypotheses of a seed's very first fit (:308-312)
constexpr int RITER = 100;
constexpr float ERR_THR = 0.7f;     // both drivers
constexpr float INCLUDE_ABOVE = 0.05f; // includeFilter = AA > 0.05 (:276)
constexpr double GAMMA0 = 0.01, GAMMA_SHRINK = 0.8;
constexpr int MAX_SEEDS = 65535;

struct Size {
    int r, c;
};

// NULL when the arguments are acceptable, else what is wrong with them, formatted into buf (the caller prefixes its own name).
inline const char *check_args(char *buf, size_t cap, int nrows, int ncols, int order, double sigmaLim, const double *cset_vect, int n_cset,
                              int iterations, int seeds, double scl_factor, double pyr_scl)
{
    if (nrows < 3 || ncols < 3) return std::snprintf(buf, cap, "D must be at least 3x3 (got %dx%d)", nrows, ncols), buf;
    if (seeds < 1 || seeds > MAX_SEEDS) return std::snprintf(buf, cap, "seeds must lie in 1..%d (got %d)", MAX_SEEDS, seeds), buf;
    if ((long long)nrows * ncols > 0x7fffffffLL / 8 || (long long)nrows * ncols * seeds > 0x7fffffffLL / 8)
        return std::snprintf(buf, cap, "planes too large"), buf;
    if (iterations < 0) return std::snprintf(buf, cap, "iterations must be >= 0 (got %d)", iterations), buf;
    if (order != 1 && order != 2)
        return std::snprintf(buf, cap, "only 1st and 2nd order polynomials are implemented (order = %d)", order), buf;
    if (!std::isfinite(sigmaLim) || sigmaLim <= 0.0) return std::snprintf(buf, cap, "sigmaLim must be finite and > 0 (got %g)", sigmaLim), buf;
    if (cset_vect == nullptr || n_cset < 1) return std::snprintf(buf, cap, "cset_vect needs at least one entry (n_cset = %d)", n_cset), buf;
    for (int i = 0; i < n_cset; i++)
        if (!std::isfinite(cset_vect[i])) return std::snprintf(buf, cap, "cset_vect[%d] is not finite", i), buf;
    if (!(scl_factor > 0.0 && scl_factor < 1.0)) return std::snprintf(buf, cap, "scl_factor must lie in (0, 1) (got %g)", scl_factor), buf;
    if (!(pyr_scl > 0.0) || !std::isfinite(pyr_scl)) return std::snprintf(buf, cap, "pyr_scl must be finite and > 0 (got %g)", pyr_scl), buf;
    return nullptr;
}

// Sizes of the scales 1..K, the rule of pdeip_region_competition: ceil(size*scl_factor) while both sides stay >= pyr_scl x the
// original (and >= 3, and still shrink).
inline std::vector<Size> scale_sizes(int nrows, int ncols, double scl_factor, double pyr_scl)
{
    std::vector<Size> sz{{nrows, ncols}};
    for (;;) {
        const int r = (int)std::ceil(sz.back().r * scl_factor), c = (int)std::ceil(sz.back().c * scl_factor);
        if (!((double)r >= nrows * pyr_scl && (double)c >= ncols * pyr_scl) || r < 3 || c < 3) break;
        if (r == sz.back().r && c == sz.back().c) break;
        sz.push_back({r, c});
    }
    return sz;
}

// Visit v = 0..2K-1 works on scale (0-based) 0..K-1, K-1..0.
inline int visit_scale(int v, int K) { return v < K ? v : 2 * K - 1 - v; }

// Hypotheses and consensus-set size of iteration `it` (1-based) of visit v.
inline int riter(int it, int v) { return it <= 1 && v == 0 ? RITER_FIRST : RITER; }
inline double rcons(const double *cset_vect, int n_cset, int it, int v)
{
    if (v != 0) return cset_vect[n_cset - 1];
    return cset_vect[(it <= n_cset ? it : n_cset) - 1];
}

inline float nu_of(double gamma, int r, int c) { return (float)(gamma * std::pow((double)r * (double)c, 0.7)); }

// The constants in which the two drivers' generateSeeds() differ; a NaN member of the caller's struct keeps the dense value.
struct Prm {
    double dist_cap, mincov_gate;
    float nan_fill;
};
inline Prm resolve(const double *dist_cap, const double *nan_fill, const double *mincov_gate)
{
    Prm p{std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity(), std::numeric_limits<float>::quiet_NaN()};
    if (dist_cap && !std::isnan(*dist_cap)) p.dist_cap = *dist_cap;
    if (nan_fill && !std::isnan(*nan_fill)) p.nan_fill = (float)*nan_fill;
    if (mincov_gate && !std::isnan(*mincov_gate)) p.mincov_gate = *mincov_gate;
    return p;
}

// ---- the dense driver (DispSegmentation.m:40-56) ----
struct DriverPrm {
    double srem_thr, scl_factor, gen_scl, rc_scl, ransac_min_cset, ransac_max_cset;
    int polyorder, seeds, ransac_cset_cycles;
};
inline DriverPrm driver_defaults() { return DriverPrm{0.002, 0.7, 0.2, 0.4, 0.1, 0.7, 1, 15, 10}; }

// cset_vect = min + (max - min)/cycles * [0:cycles]  (:56)
inline std::vector<double> cset_vector(double lo, double hi, int cycles)
{
    std::vector<double> v((size_t)cycles + 1);
    const double step = (hi - lo) / cycles;
    for (int i = 0; i <= cycles; i++) v[(size_t)i] = lo + step * (double)i;
    return v;
}

inline const char *check_driver(char *buf, size_t cap, const DriverPrm &p)
{
    if (!std::isfinite(p.srem_thr)) return std::snprintf(buf, cap, "srem_thr must be finite"), buf;
    if (p.seeds < 1 || p.seeds > MAX_SEEDS / 2) return std::snprintf(buf, cap, "seeds must lie in 1..%d (got %d)", MAX_SEEDS / 2, p.seeds), buf;
    if (p.ransac_cset_cycles < 1 || p.ransac_cset_cycles > 65535)
        return std::snprintf(buf, cap, "ransac_cset_cycles must lie in 1..65535 (got %d)", p.ransac_cset_cycles), buf;
    if (!std::isfinite(p.ransac_min_cset) || !std::isfinite(p.ransac_max_cset))
        return std::snprintf(buf, cap, "ransac_min_cset and ransac_max_cset must be finite"), buf;
    if (!(p.gen_scl > 0.0) || !std::isfinite(p.gen_scl)) return std::snprintf(buf, cap, "gen_scl must be finite and > 0 (got %g)", p.gen_scl), buf;
    if (!(p.rc_scl > 0.0) || !std::isfinite(p.rc_scl)) return std::snprintf(buf, cap, "rc_scl must be finite and > 0 (got %g)", p.rc_scl), buf;
    return nullptr;
}

// Stage j (0-based, in call order) of the driver draws from seed + j*2^32 (64-bit wrapping).
inline unsigned long long stage_seed(unsigned long long seed, int j) { return seed + ((unsigned long long)j << 32); }

} // namespace seeds
} // namespace pdeip
