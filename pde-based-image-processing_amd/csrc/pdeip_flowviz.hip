// pdeip_flowviz.hip -- libpdeip.so: looking at a flow field and scoring it where it lies.
//
//   img = flow2color(cat(3, U, V), 'maxvalue', m, 'border', b) (matlab/optical_flow/flow2color.m)   pdeip_flow2color(_dev)
//   endpoint error and Barron's angular error against a ground truth, with their means                pdeip_flow_errors(_dev)
//
// Kernels: csrc/pdeip_flowviz.hpp; the contract: include/pdeip.h.  Neither call has an ordering, so pdeip_set_mode does not apply.
// Nothing is read back in the _dev forms: the automatic maximum stays in a device cell between the launches.
//
// Build (build.py): hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -c, one object per translation unit.
#include "pdeip_ctx.hpp"
#include "pdeip_flowviz.hpp"

#include <cmath>

using namespace pdeip;
using namespace pdeip::flowviz;

namespace {

// Workspace (WS_FLOWVIZ): the maximum's cell, then the error partials [4][ntiles] doubles.
constexpr size_t CELL_BYTES = 16;

// Everything refused is refused here, before any HIP call.
int color_args(const char *who, const void *U, const void *V, int nrows, int ncols, int border, const void *rgb_out, const void *rgb8_out)
{
    NONNULL(who, U); NONNULL(who, V);
    if (rgb_out == nullptr && rgb8_out == nullptr) return set_err(PDEIP_ERR_ARG, "%s: rgb_out and rgb8_out are both NULL", who);
    if (nrows < 1 || ncols < 1) return set_err(PDEIP_ERR_ARG, "%s: the field must be at least 1x1 (got %dx%d)", who, nrows, ncols);
    if (border < 0) return set_err(PDEIP_ERR_ARG, "%s: border must be >= 0 (got %d)", who, border);
    const long long brows = (long long)nrows + 2LL * border, bcols = (long long)ncols + 2LL * border;
    if (brows > 0x7fffffffLL || bcols > 0x7fffffffLL || brows * bcols * 3 > 0x7fffffffLL)
        return set_err(PDEIP_ERR_ARG, "%s: the picture has more than 2^31-1 elements", who);
    if ((bcols + TILE_SIDE - 1) / TILE_SIDE > 65535)
        return set_err(PDEIP_ERR_UNSUPPORTED, "%s: more than %d columns with the border (got %lld)", who, 65535 * TILE_SIDE, bcols);
    return PDEIP_OK;
}

int error_args(const char *who, const void *U, const void *V, const void *Ut, const void *Vt, int nrows, int ncols, const void *stats_out)
{
    NONNULL(who, U); NONNULL(who, V); NONNULL(who, Ut); NONNULL(who, Vt); NONNULL(who, stats_out);
    if (nrows < 1 || ncols < 1) return set_err(PDEIP_ERR_ARG, "%s: the field must be at least 1x1 (got %dx%d)", who, nrows, ncols);
    if ((long long)nrows * ncols > 0x7fffffffLL) return set_err(PDEIP_ERR_ARG, "%s: more than 2^31-1 elements", who);
    return PDEIP_OK;
}

inline int err_tiles(size_t n) { return (int)((n + ERR_TILE - 1) / ERR_TILE); }

} // namespace

// Launches: 1 when maxvalue is given; 3 (cell, maximum, colours) when it is NaN.  Never depends on the data.
extern "C" int pdeip_flow2color_dev(void *stream, const float *U, const float *V, int nrows, int ncols, double maxvalue, int border,
                                    float *rgb_out, unsigned char *rgb8_out, double *maxvalue_out)
{
    const char *who = "pdeip_flow2color_dev";
    RC(color_args(who, U, V, nrows, ncols, border, rgb_out, rgb8_out));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t n = (size_t)nrows * ncols;
    unsigned long long *cell = nullptr;
    int launches = 0;
    if (std::isnan(maxvalue)) {
        float *ws = nullptr;
        RC(ws_get(WS_FLOWVIZ, CELL_BYTES, &ws));
        cell = reinterpret_cast<unsigned long long *>(ws);
        const size_t want = (n + BLOCK - 1) / BLOCK;
        const unsigned blocks = (unsigned)(want < (size_t)MAXMAG_BLOCKS ? want : (size_t)MAXMAG_BLOCKS);
        hipLaunchKernelGGL(k_flow_cell_init, dim3(1), dim3(64), 0, s, cell);
        hipLaunchKernelGGL(k_flow_maxmag, dim3(blocks), dim3(BLOCK), 0, s, U, V, n, aligned16(U) && aligned16(V) ? 1 : 0, cell);
        launches += 2;
    }
    const int brows = nrows + 2 * border, bcols = ncols + 2 * border;
    const dim3 grid((unsigned)((brows + TILE_SIDE - 1) / TILE_SIDE), (unsigned)((bcols + TILE_SIDE - 1) / TILE_SIDE));
    hipLaunchKernelGGL(k_flow2color, grid, dim3(BLOCK), 0, s, U, V, nrows, ncols, border, maxvalue, cell, rgb_out, rgb8_out, maxvalue_out);
    HIPCHK(hipGetLastError());
    tls.last_launches = launches + 1;
    return PDEIP_OK;
}

extern "C" int pdeip_flow2color(const float *U, const float *V, int nrows, int ncols, double maxvalue, int border, float *rgb_out,
                                unsigned char *rgb8_out, double *maxvalue_out)
{
    const char *who = "pdeip_flow2color";
    RC(color_args(who, U, V, nrows, ncols, border, rgb_out, rgb8_out));
    RC(use_device());
    const size_t n = (size_t)nrows * ncols, bn = (size_t)(nrows + 2 * border) * (size_t)(ncols + 2 * border);
    // arena: the maximum (a double, padded to 16 bytes), U, V, the float picture, the uint8 picture
    const size_t floats = 4 + 2 * pad4(n) + (rgb_out ? pad4(3 * bn) : 0);
    float *ar = nullptr;
    RC(ws_get(WS_ARENA, floats * sizeof(float) + (rgb8_out ? 3 * bn : 0), &ar));
    double *dmax = reinterpret_cast<double *>(ar);
    float *dU = ar + 4, *dV = dU + pad4(n), *drgb = rgb_out ? dV + pad4(n) : nullptr;
    unsigned char *drgb8 = rgb8_out ? reinterpret_cast<unsigned char *>(ar + floats) : nullptr;
    HIPCHK(hipMemcpy(dU, U, n * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dV, V, n * sizeof(float), hipMemcpyHostToDevice));
    RC(pdeip_flow2color_dev(nullptr, dU, dV, nrows, ncols, maxvalue, border, drgb, drgb8, dmax));
    if (rgb_out) HIPCHK(hipMemcpy(rgb_out, drgb, 3 * bn * sizeof(float), hipMemcpyDeviceToHost));
    if (rgb8_out) HIPCHK(hipMemcpy(rgb8_out, drgb8, 3 * bn, hipMemcpyDeviceToHost));
    if (maxvalue_out) HIPCHK(hipMemcpy(maxvalue_out, dmax, sizeof(double), hipMemcpyDeviceToHost));
    return PDEIP_OK;
}

// Launches: 2 (tiles, final).
extern "C" int pdeip_flow_errors_dev(void *stream, const float *U, const float *V, const float *Ut, const float *Vt, const float *mask,
                                     int nrows, int ncols, float *epe_out, float *ang_out, double *stats_out)
{
    const char *who = "pdeip_flow_errors_dev";
    RC(error_args(who, U, V, Ut, Vt, nrows, ncols, stats_out));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t n = (size_t)nrows * ncols;
    const int ntiles = err_tiles(n);
    float *ws = nullptr;
    RC(ws_get(WS_FLOWVIZ, CELL_BYTES + 4 * (size_t)ntiles * sizeof(double), &ws));
    double *partials = reinterpret_cast<double *>(reinterpret_cast<char *>(ws) + CELL_BYTES);
    hipLaunchKernelGGL(k_flow_err_tiles, dim3((unsigned)ntiles), dim3(BLOCK), 0, s, U, V, Ut, Vt, mask, n, epe_out, ang_out, partials);
    hipLaunchKernelGGL(k_flow_err_final, dim3(1), dim3(BLOCK), 0, s, partials, ntiles, stats_out);
    HIPCHK(hipGetLastError());
    tls.last_launches = 2;
    return PDEIP_OK;
}

extern "C" int pdeip_flow_errors(const float *U, const float *V, const float *Ut, const float *Vt, const float *mask, int nrows, int ncols,
                                 float *epe_out, float *ang_out, double *stats_out)
{
    const char *who = "pdeip_flow_errors";
    RC(error_args(who, U, V, Ut, Vt, nrows, ncols, stats_out));
    RC(use_device());
    const size_t n = (size_t)nrows * ncols, pn = pad4(n);
    // arena: the statistics (four doubles), then U, V, Ut, Vt, mask, epe, ang
    float *ar = nullptr;
    RC(ws_get(WS_ARENA, (8 + 7 * pn) * sizeof(float), &ar));
    double *dstats = reinterpret_cast<double *>(ar);
    float *in[5] = {ar + 8, ar + 8 + pn, ar + 8 + 2 * pn, ar + 8 + 3 * pn, mask ? ar + 8 + 4 * pn : nullptr};
    const float *src[5] = {U, V, Ut, Vt, mask};
    for (int k = 0; k < 5; k++)
        if (src[k]) HIPCHK(hipMemcpy(in[k], src[k], n * sizeof(float), hipMemcpyHostToDevice));
    float *depe = epe_out ? ar + 8 + 5 * pn : nullptr, *dang = ang_out ? ar + 8 + 6 * pn : nullptr;
    RC(pdeip_flow_errors_dev(nullptr, in[0], in[1], in[2], in[3], in[4], nrows, ncols, depe, dang, dstats));
    if (epe_out) HIPCHK(hipMemcpy(epe_out, depe, n * sizeof(float), hipMemcpyDeviceToHost));
    if (ang_out) HIPCHK(hipMemcpy(ang_out, dang, n * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(stats_out, dstats, 4 * sizeof(double), hipMemcpyDeviceToHost));
    return PDEIP_OK;
}
