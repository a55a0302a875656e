// pdeip_ccl.hip -- libpdeip.so: connected-component labelling, the piece of generateSeeds() that is no composition of the others.
//
//   [L, num] = bwlabel(A > 0, conn), regionprops(.., 'Area')     pdeip_bwlabel(_dev)
//   the largest component as a two-valued plane                  pdeip_largest_component(_dev)   (DispSegmentation.m:282-298)
//
// Kernels: csrc/pdeip_ccl.hpp; what a call decides on the host: csrc/pdeip_ccl_plan.hpp; the contract: include/pdeip.h.
// pdeip_set_mode does not apply.  PDEIP_CCL_SMALL=0|1 forces the tiled / the one-workgroup form (1: wherever it admits the plane).
//
// Build (build.py): hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -c, one object per translation unit.
#include "pdeip_ctx.hpp"
#include "pdeip_ccl.hpp"

using namespace pdeip;
using namespace pdeip::ccl;

namespace {

int check(const char *who, const void *A, const void *out, int nrows, int ncols, int conn, int areas_cap)
{
    const char *bad = check_args(A, out, nrows, ncols, conn, areas_cap);
    return bad ? set_err(PDEIP_ERR_ARG, "%s: %s (nrows %d, ncols %d, conn %d, areas_cap %d)", who, bad, nrows, ncols, conn, areas_cap) : PDEIP_OK;
}

// Labels the plane.  L_out / num_out / areas_out (cap areas_cap) as pdeip_bwlabel_dev; with sel_out the two-valued plane of the
// largest component and its area (then L_out and areas_out are NULL and the tiled form takes both from the workspace).
int run(hipStream_t s, const float *A, int nrows, int ncols, int conn, int *L_out, int *num_out, int *areas_out, int areas_cap, float *sel_out,
        float hi, float lo, int *best_area_out)
{
    const Plan pl = make_plan(nrows, ncols, env_int("PDEIP_CCL_SMALL", -1));
    const int conn8 = conn == 8 ? 1 : 0;
    if (pl.small) {
        RC(ensure_lds(reinterpret_cast<const void *>(k_ccl_small), pl.small_lds));
        hipLaunchKernelGGL(k_ccl_small, dim3(1), dim3(SMALL_THREADS), pl.small_lds, s, A, nrows, ncols, conn8, (int)pad4z((size_t)pl.npix), L_out, num_out,
                           areas_out, areas_cap, sel_out, hi, lo, best_area_out);
        HIPCHK(hipGetLastError());
        tls.last_launches = 1;
        return PDEIP_OK;
    }
    float *wsf = nullptr;
    RC(ws_get(WS_CCL, pl.ws_ints * sizeof(int), &wsf));
    int *ws = reinterpret_cast<int *>(wsf);
    int *T = ws + pl.off_tree, *blk = ws + pl.off_blk, *scal = ws + pl.off_scalars;
    int *L = L_out, *areas = areas_out, cap = areas_cap;
    if (sel_out) {
        L = ws + pl.off_labels;
        areas = ws + pl.off_areas;
        cap = pl.max_labels;
    }
    int launches = 0;
    if (cap <= 0) areas = nullptr;
    hipLaunchKernelGGL(k_ccl_local, dim3((unsigned)(pl.tiles_i * pl.tiles_j)), dim3(TILE_THREADS), 0, s, A, nrows, ncols, pl.tiles_i, conn8, T);
    launches++;
    if (pl.seam_items > 0) {
        hipLaunchKernelGGL(k_ccl_seam, dim3((unsigned)pl.seam_blocks), dim3(LIN_THREADS), 0, s, T, nrows, ncols, conn8,
                           (pl.tiles_j - 1) * nrows, pl.seam_items);
        launches++;
    }
    const dim3 lin((unsigned)pl.lin_blocks), lt(LIN_THREADS);
    hipLaunchKernelGGL(k_ccl_flatten, lin, lt, 0, s, T, pl.npix, blk, areas, cap);
    hipLaunchKernelGGL(k_ccl_scan, dim3(1), dim3(SCAN_THREADS), 0, s, blk, pl.lin_blocks, scal, sel_out ? nullptr : num_out);
    hipLaunchKernelGGL(k_ccl_rank, lin, lt, 0, s, T, pl.npix, blk, L);
    hipLaunchKernelGGL(k_ccl_relabel, lin, lt, 0, s, T, pl.npix, L, areas, cap);
    launches += 4;
    if (sel_out) {
        hipLaunchKernelGGL(k_ccl_argmax, dim3(1), dim3(ARG_THREADS), 0, s, areas, scal, scal + 1);
        hipLaunchKernelGGL(k_ccl_select, lin, lt, 0, s, L, pl.npix, scal + 1, scal, hi, lo, sel_out, num_out, best_area_out);
        launches += 2;
    }
    HIPCHK(hipGetLastError());
    tls.last_launches = launches;
    return PDEIP_OK;
}

} // namespace

extern "C" int pdeip_bwlabel_dev(void *stream, const float *A, int nrows, int ncols, int conn, int *L_out, int *num_out, int *areas_out,
                                 int areas_cap)
{
    const char *who = "pdeip_bwlabel_dev";
    RC(check(who, A, L_out, nrows, ncols, conn, areas_cap));
    NONNULL(who, num_out);
    if (reinterpret_cast<const void *>(L_out) == reinterpret_cast<const void *>(A)) return set_err(PDEIP_ERR_ARG, "%s: L_out must not alias A", who);
    return run(static_cast<hipStream_t>(stream), A, nrows, ncols, conn, L_out, num_out, areas_out, areas_out ? areas_cap : 0, nullptr, 0.0f, 0.0f, nullptr);
}

extern "C" int pdeip_largest_component_dev(void *stream, const float *A, int nrows, int ncols, int conn, float hi, float lo, float *out, int *num_out,
                                           int *area_out)
{
    const char *who = "pdeip_largest_component_dev";
    RC(check(who, A, out, nrows, ncols, conn, 0));
    return run(static_cast<hipStream_t>(stream), A, nrows, ncols, conn, nullptr, num_out, nullptr, 0, out, hi, lo, area_out);
}

extern "C" int pdeip_bwlabel(const float *A, int nrows, int ncols, int conn, int *L_out, int *num_out, int *areas_out, int areas_cap)
{
    const char *who = "pdeip_bwlabel";
    RC(check(who, A, L_out, nrows, ncols, conn, areas_cap));
    NONNULL(who, num_out);
    RC(use_device());
    const size_t n = (size_t)nrows * ncols, na = areas_out ? (size_t)areas_cap : 0;
    float *ar = nullptr;
    RC(ws_get(WS_ARENA, (2 * pad4(n) + 4 + pad4(na)) * sizeof(float), &ar));
    int *dL = reinterpret_cast<int *>(ar + pad4(n)), *dNum = dL + pad4(n), *dAreas = dNum + 4;
    HIPCHK(hipMemcpy(ar, A, n * sizeof(float), hipMemcpyHostToDevice));
    RC(pdeip_bwlabel_dev(nullptr, ar, nrows, ncols, conn, dL, dNum, na ? dAreas : nullptr, (int)na));
    HIPCHK(hipMemcpy(L_out, dL, n * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(num_out, dNum, sizeof(int), hipMemcpyDeviceToHost));
    if (na) HIPCHK(hipMemcpy(areas_out, dAreas, na * sizeof(int), hipMemcpyDeviceToHost));
    return PDEIP_OK;
}

extern "C" int pdeip_largest_component(const float *A, int nrows, int ncols, int conn, float hi, float lo, float *out, int *num_out, int *area_out)
{
    const char *who = "pdeip_largest_component";
    RC(check(who, A, out, nrows, ncols, conn, 0));
    RC(use_device());
    const size_t n = (size_t)nrows * ncols;
    float *ar = nullptr;
    RC(ws_get(WS_ARENA, (pad4(n) + 4) * sizeof(float), &ar));
    int *dScal = reinterpret_cast<int *>(ar + pad4(n));
    HIPCHK(hipMemcpy(ar, A, n * sizeof(float), hipMemcpyHostToDevice));
    RC(pdeip_largest_component_dev(nullptr, ar, nrows, ncols, conn, hi, lo, ar, dScal, dScal + 1));
    HIPCHK(hipMemcpy(out, ar, n * sizeof(float), hipMemcpyDeviceToHost));
    if (num_out) HIPCHK(hipMemcpy(num_out, dScal, sizeof(int), hipMemcpyDeviceToHost));
    if (area_out) HIPCHK(hipMemcpy(area_out, dScal + 1, sizeof(int), hipMemcpyDeviceToHost));
    return PDEIP_OK;
}
