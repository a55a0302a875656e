// pdeip_ccl_plan.hpp -- what a connected-component call decides on the host before any HIP call: the argument checks, which of
// the two forms runs, the launch geometry and the workspace layout.  Plain C++ (no HIP, no library state), so that
// tools/ccl_plan_check.cpp can run it under the host sanitizers; csrc/pdeip_ccl.hip is its only other user.
#pragma once
#include <climits>
#include <cstddef>

namespace pdeip {
namespace ccl {

constexpr int TILE_I = 64;                    // rows of a tile: one wave runs down a tile column
constexpr int TILE_J = 32;                    // columns of a tile
constexpr int TILE_THREADS = 256;             // 4 waves, 8 tile columns each
constexpr int LIN_THREADS = 256;              // the kernels over pixels in memory order
constexpr int LIN_PER_THREAD = 4;
constexpr int LIN_PIX = LIN_THREADS * LIN_PER_THREAD; // pixels of one such block: the unit of the root-rank scan
constexpr int HASH_SLOTS = 2 * LIN_PIX;       // (block, label) area table: at most LIN_PIX distinct labels per block
constexpr int SCAN_THREADS = 256;
constexpr int SMALL_THREADS = 1024;           // the one workgroup of the small form
constexpr int SMALL_WAVES = SMALL_THREADS / 64;
constexpr int SMALL_MAX_PIX = 16384;          // two int planes in LDS: 128 KiB of the CU's 160
constexpr int ARG_THREADS = 1024;             // the single workgroup that picks the largest area

// NULL when the arguments are acceptable, else what is wrong with them (the caller prefixes its own name).
inline const char *check_args(const void *A, const void *out, int nrows, int ncols, int conn, int areas_cap)
{
    if (A == nullptr) return "argument 'A' is NULL";
    if (out == nullptr) return "an output argument is NULL";
    if (nrows < 1 || ncols < 1) return "nrows and ncols must be >= 1";
    if ((long long)nrows * (long long)ncols > (long long)INT_MAX) return "nrows*ncols exceeds INT_MAX";
    if (conn != 4 && conn != 8) return "conn must be 4 or 8";
    if (areas_cap < 0) return "areas_cap must be >= 0";
    return nullptr;
}

struct Plan {
    bool small;       // one launch of k_ccl_small
    int npix;
    int tiles_i, tiles_j; // grid of k_ccl_local
    int seam_items;   // pixels on the inner tile borders: (tiles_j - 1) columns of nrows + (tiles_i - 1) rows of ncols
    int seam_blocks;  // blocks of LIN_THREADS of them
    int lin_blocks;   // blocks of LIN_PIX pixels
    int max_labels;   // no mask has more components than this
    size_t small_lds; // dynamic LDS bytes of k_ccl_small
    // workspace of the tiled form, in ints from the base: the tree plane, the block counts, a label plane and an area table (the
    // last two only when the caller gave none: pdeip_largest_component_dev), the scalars {num, best label, best area}
    size_t off_tree, off_blk, off_labels, off_areas, off_scalars, ws_ints;
};

inline size_t pad4z(size_t n) { return (n + 3) & ~(size_t)3; }

// force_small: -1 decide by size, 0 the tiled form, 1 the small form wherever it admits the plane (PDEIP_CCL_SMALL).
inline Plan make_plan(int nrows, int ncols, int force_small)
{
    Plan p{};
    p.npix = nrows * ncols;
    const bool admits = p.npix <= SMALL_MAX_PIX;
    p.small = admits && force_small != 0;
    p.tiles_i = (int)(((long long)nrows + TILE_I - 1) / TILE_I);
    p.tiles_j = (int)(((long long)ncols + TILE_J - 1) / TILE_J);
    p.seam_items = (int)((long long)(p.tiles_j - 1) * nrows + (long long)(p.tiles_i - 1) * ncols); // < npix
    p.seam_blocks = (int)(((long long)p.seam_items + LIN_THREADS - 1) / LIN_THREADS);
    p.lin_blocks = (int)(((long long)p.npix + LIN_PIX - 1) / LIN_PIX);
    p.max_labels = (int)(((long long)p.npix + 1) / 2); // the checkerboard under conn 4
    p.small_lds = (2 * pad4z((size_t)p.npix)) * sizeof(int);
    p.off_tree = 0;
    p.off_blk = p.off_tree + pad4z((size_t)p.npix);
    p.off_labels = p.off_blk + pad4z((size_t)p.lin_blocks);
    p.off_areas = p.off_labels + pad4z((size_t)p.npix);
    p.off_scalars = p.off_areas + pad4z((size_t)p.max_labels);
    p.ws_ints = p.off_scalars + 4;
    return p;
}

} // namespace ccl
} // namespace pdeip
