// pdeip_sparse.hip -- libpdeip.so: what DispSegmentationSparse.m adds to the dense driver's stages.
//
//   nanmedfilt2() (DispSegmentationSparse.m:679-685)                       pdeip_nanmedfilt2(_dev)
//   the D pyramid of :63-64, :76-79                                        pdeip_sparse_pyramid, sparse_pyramid_dev (library-internal)
//
// Kernel: csrc/pdeip_sparse.hpp; the host-side plan: csrc/pdeip_sparse_plan.hpp; the contract: include/pdeip.h.  The stages that
// use the pyramid (pdeip_generate_seeds_sparse, pdeip_region_competition_sparse) and the driver are in csrc/pdeip_segmentation.hip.
// pdeip_set_mode does not apply.
//
// Build (build.py): hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -c, one object per translation unit.
#include "pdeip_ctx.hpp"
#include "pdeip_sparse.hpp"
#include "pdeip_sparse_plan.hpp"

using namespace pdeip;

namespace {

int check_filter(const char *who, const void *A, const void *out, int nrows, int ncols, int nframes)
{
    char buf[160];
    bool unsupported = false;
    const char *bad = sparse::check_filter(buf, sizeof buf, A, out, nrows, ncols, nframes, &unsupported);
    return bad ? set_err(unsupported ? PDEIP_ERR_UNSUPPORTED : PDEIP_ERR_ARG, "%s: %s", who, bad) : PDEIP_OK;
}

int launch_nanmedian(hipStream_t s, const float *A, int nrows, int ncols, int nframes, float *out)
{
    hipLaunchKernelGGL(k_nanmedian3, pixel_grid(nrows, ncols, nframes), dim3(256), 0, s, out, A, nrows, ncols);
    HIPCHK(hipGetLastError());
    return PDEIP_OK;
}

} // namespace

extern "C" int pdeip_nanmedfilt2_dev(void *stream, const float *A, int nrows, int ncols, int nframes, float *out)
{
    RC(check_filter("pdeip_nanmedfilt2_dev", A, out, nrows, ncols, nframes));
    RC(launch_nanmedian(static_cast<hipStream_t>(stream), A, nrows, ncols, nframes, out));
    tls.last_launches = 1;
    return PDEIP_OK;
}

extern "C" int pdeip_nanmedfilt2(const float *A, int nrows, int ncols, int nframes, float *out)
{
    const char *who = "pdeip_nanmedfilt2";
    RC(check_filter(who, A, out, nrows, ncols, nframes));
    RC(use_device());
    const size_t n = (size_t)nrows * ncols * nframes;
    float *ar = nullptr;
    RC(ws_get(WS_ARENA, 2 * pad4(n) * sizeof(float), &ar));
    HIPCHK(hipMemcpy(ar, A, n * sizeof(float), hipMemcpyHostToDevice));
    RC(launch_nanmedian(nullptr, ar, nrows, ncols, nframes, ar + pad4(n)));
    HIPCHK(hipMemcpy(out, ar + pad4(n), n * sizeof(float), hipMemcpyDeviceToHost));
    tls.last_launches = 1;
    return PDEIP_OK;
}

// P[0] = nanmed(D); P[k] = nanmed(resize_cubic(nanmed(P[k-1]))): 3K - 2 launches on s, nothing read back.  rc holds rows, cols per
// scale; t1 holds a plane of scale 1, t2 one of scale 2 (sparse::layout); D must not be P[0].
int pdeip::sparse_pyramid_dev(hipStream_t s, const float *D, const int *rc, int K, float *const *P, float *t1, float *t2)
{
    RC(launch_nanmedian(s, D, rc[0], rc[1], 1, P[0]));
    for (int k = 1; k < K; k++) {
        const int r0 = rc[2 * k - 2], c0 = rc[2 * k - 1], r = rc[2 * k], c = rc[2 * k + 1];
        RC(launch_nanmedian(s, P[k - 1], r0, c0, 1, t1));
        RC(pdeip_pyr_resize_dev(s, t1, r0, c0, 1, r, c, 1, t2));
        RC(launch_nanmedian(s, t2, r, c, 1, P[k]));
    }
    return PDEIP_OK;
}

extern "C" int pdeip_sparse_pyramid(const float *D, int nrows, int ncols, double scl_factor, double pyr_scl, int scales_cap, int *K_out,
                                    int *sizes_out, float *out)
{
    const char *who = "pdeip_sparse_pyramid";
    tls.err[0] = '\0';
    NONNULL(who, K_out); NONNULL(who, sizes_out);
    if (out != nullptr) NONNULL(who, D);
    {
        char buf[160];
        const char *bad = sparse::check_pyramid(buf, sizeof buf, nrows, ncols, scl_factor, pyr_scl, scales_cap);
        if (bad) return set_err(PDEIP_ERR_ARG, "%s: %s", who, bad);
    }
    if (ncols > sparse::MAX_GRID_YZ) return set_err(PDEIP_ERR_UNSUPPORTED, "%s: more than %d columns (got %d)", who, sparse::MAX_GRID_YZ, ncols);
    const std::vector<seeds::Size> sz = seeds::scale_sizes(nrows, ncols, scl_factor, pyr_scl);
    const int K = (int)sz.size();
    if (K > scales_cap) return set_err(PDEIP_ERR_ARG, "%s: the pyramid has %d scales but scales_cap is %d", who, K, scales_cap);
    if (out != nullptr) {
        const sparse::Layout L = sparse::layout(sz);
        const size_t n0 = sparse::pixels(sz[0]);
        RC(use_device());
        float *ar = nullptr;
        RC(ws_get(WS_ARENA, (L.total + pad4(n0)) * sizeof(float), &ar));
        float *Draw = ar + L.total;
        std::vector<float *> P((size_t)K);
        std::vector<int> rc((size_t)2 * K);
        for (int k = 0; k < K; k++) {
            P[(size_t)k] = ar + L.scale[(size_t)k];
            rc[(size_t)2 * k] = sz[(size_t)k].r;
            rc[(size_t)2 * k + 1] = sz[(size_t)k].c;
        }
        HIPCHK(hipMemcpy(Draw, D, n0 * sizeof(float), hipMemcpyHostToDevice));
        RC(sparse_pyramid_dev(nullptr, Draw, rc.data(), K, P.data(), ar + L.t1, ar + L.t2));
        size_t at = 0;
        for (int k = 0; k < K; k++) {
            HIPCHK(hipMemcpy(out + at, P[(size_t)k], sparse::pixels(sz[(size_t)k]) * sizeof(float), hipMemcpyDeviceToHost));
            at += sparse::pixels(sz[(size_t)k]);
        }
        tls.last_launches = L.launches;
    }
    *K_out = K;
    for (int k = 0; k < K; k++) {
        sizes_out[2 * k] = sz[(size_t)k].r;
        sizes_out[2 * k + 1] = sz[(size_t)k].c;
    }
    return PDEIP_OK;
}
