// pdeip_crosscheck.hip -- libpdeip.so: where a computed disparity or flow can be trusted.
//
//   the left-right check of the two disparities of the symmetric stereo driver: mask, sparse map, statistics   pdeip_disp_crosscheck(_dev)
//   the forward-backward check of two flows (Sundaram, Brox, Keutzer, ECCV 2010): mask, error, statistics      pdeip_flow_crosscheck(_dev)
//
// Kernels: csrc/pdeip_crosscheck.hpp; the contract: include/pdeip.h.  Neither call has an ordering, so pdeip_set_mode does not apply.
// Nothing is read back in the _dev forms: the workgroups' partials stay in the workspace between the two launches.
//
// Build (build.py): hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -c, one object per translation unit.
#include "pdeip_ctx.hpp"
#include "pdeip_crosscheck.hpp"

#include <cmath>

using namespace pdeip;
using namespace pdeip::crosscheck;

namespace {

constexpr int MAX_GRID_Y = 65535; // the column is blockIdx.y

// Everything refused is refused here, before any HIP call.
int shape_args(const char *who, int nrows, int ncols, int min_rows)
{
    if (nrows < min_rows || ncols < 2)
        return set_err(PDEIP_ERR_ARG, "%s: the field must be at least %dx2 (got %dx%d)", who, min_rows, nrows, ncols);
    if ((long long)nrows * ncols > 0x7fffffffLL) return set_err(PDEIP_ERR_ARG, "%s: more than 2^31-1 elements", who);
    if (ncols > MAX_GRID_Y) return set_err(PDEIP_ERR_UNSUPPORTED, "%s: more than %d columns (got %d)", who, MAX_GRID_Y, ncols);
    return PDEIP_OK;
}

int threshold_arg(const char *who, const char *name, double v)
{
    if (!(v >= 0.0)) return set_err(PDEIP_ERR_ARG, "%s: %s must be >= 0 and not NaN (got %g)", who, name, v);
    return PDEIP_OK;
}

int alias_arg(const char *who, const char *out_name, const void *out, const char *in_name, const void *in)
{
    if (out != nullptr && out == in) return set_err(PDEIP_ERR_ARG, "%s: %s is the gathered plane %s", who, out_name, in_name);
    return PDEIP_OK;
}

int disp_args(const char *who, const void *D0, const void *D1, int nrows, int ncols, double tol, const void *sparse_out, const void *mask_out,
              const void *diff_out, const void *stats_out)
{
    NONNULL(who, D0); NONNULL(who, D1);
    if (sparse_out == nullptr && mask_out == nullptr && diff_out == nullptr && stats_out == nullptr)
        return set_err(PDEIP_ERR_ARG, "%s: sparse_out, mask_out, diff_out and stats_out are all NULL", who);
    RC(shape_args(who, nrows, ncols, 1));
    RC(threshold_arg(who, "tol", tol));
    RC(alias_arg(who, "sparse_out", sparse_out, "D1", D1));
    RC(alias_arg(who, "mask_out", mask_out, "D1", D1));
    RC(alias_arg(who, "diff_out", diff_out, "D1", D1));
    RC(alias_arg(who, "stats_out", stats_out, "D1", D1));
    return PDEIP_OK;
}

int flow_args(const char *who, const void *Uf, const void *Vf, const void *Ub, const void *Vb, int nrows, int ncols, double a, double b,
              const void *mask_out, const void *err_out, const void *stats_out)
{
    NONNULL(who, Uf); NONNULL(who, Vf); NONNULL(who, Ub); NONNULL(who, Vb);
    if (mask_out == nullptr && err_out == nullptr && stats_out == nullptr)
        return set_err(PDEIP_ERR_ARG, "%s: mask_out, err_out and stats_out are all NULL", who);
    RC(shape_args(who, nrows, ncols, 2));
    RC(threshold_arg(who, "a", a));
    RC(threshold_arg(who, "b", b));
    const void *outs[3] = {mask_out, err_out, stats_out};
    const char *names[3] = {"mask_out", "err_out", "stats_out"};
    for (int k = 0; k < 3; k++) {
        RC(alias_arg(who, names[k], outs[k], "Ub", Ub));
        RC(alias_arg(who, names[k], outs[k], "Vb", Vb));
    }
    return PDEIP_OK;
}

// Workspace (WS_CROSSCHECK): the partials [4][nparts] doubles, one part per workgroup of the pixel grid.
int partials_for(dim3 grid, double **partials, int *nparts)
{
    *nparts = (int)(grid.x * grid.y); // at most ceil(nrows / 256) * ncols <= the pixel count
    float *ws = nullptr;
    RC(ws_get(WS_CROSSCHECK, 4 * (size_t)*nparts * sizeof(double), &ws));
    *partials = reinterpret_cast<double *>(ws);
    return PDEIP_OK;
}

} // namespace

// Launches: 2 (pixels, final) with stats_out, 1 without.  Never depends on the data.
extern "C" int pdeip_disp_crosscheck_dev(void *stream, const float *D0, const float *D1, int nrows, int ncols, double tol, float *sparse_out,
                                         float *mask_out, float *diff_out, double *stats_out)
{
    const char *who = "pdeip_disp_crosscheck_dev";
    RC(disp_args(who, D0, D1, nrows, ncols, tol, sparse_out, mask_out, diff_out, stats_out));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid = pixel_grid(nrows, ncols, 1);
    double *partials = nullptr;
    int nparts = 0;
    if (stats_out != nullptr) RC(partials_for(grid, &partials, &nparts));
    hipLaunchKernelGGL(k_disp_crosscheck, grid, dim3(BLOCK), 0, s, D0, D1, nrows, ncols, tol, sparse_out, mask_out, diff_out, partials);
    if (stats_out != nullptr) hipLaunchKernelGGL(k_crosscheck_final, dim3(1), dim3(FINAL_BLOCK), 0, s, partials, nparts, stats_out);
    HIPCHK(hipGetLastError());
    tls.last_launches = stats_out != nullptr ? 2 : 1;
    return PDEIP_OK;
}

extern "C" int pdeip_disp_crosscheck(const float *D0, const float *D1, int nrows, int ncols, double tol, float *sparse_out, float *mask_out,
                                     float *diff_out, double *stats_out)
{
    const char *who = "pdeip_disp_crosscheck";
    RC(disp_args(who, D0, D1, nrows, ncols, tol, sparse_out, mask_out, diff_out, stats_out));
    RC(use_device());
    const size_t n = (size_t)nrows * ncols, pn = pad4(n);
    // arena: the statistics (four doubles), then D0, D1, sparse, mask, diff
    float *ar = nullptr;
    RC(ws_get(WS_ARENA, (8 + 5 * pn) * sizeof(float), &ar));
    double *dstats = stats_out ? reinterpret_cast<double *>(ar) : nullptr;
    float *d0 = ar + 8, *d1 = d0 + pn;
    float *dsp = sparse_out ? d1 + pn : nullptr, *dmask = mask_out ? d1 + 2 * pn : nullptr, *ddiff = diff_out ? d1 + 3 * pn : nullptr;
    HIPCHK(hipMemcpy(d0, D0, n * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d1, D1, n * sizeof(float), hipMemcpyHostToDevice));
    RC(pdeip_disp_crosscheck_dev(nullptr, d0, d1, nrows, ncols, tol, dsp, dmask, ddiff, dstats));
    if (sparse_out) HIPCHK(hipMemcpy(sparse_out, dsp, n * sizeof(float), hipMemcpyDeviceToHost));
    if (mask_out) HIPCHK(hipMemcpy(mask_out, dmask, n * sizeof(float), hipMemcpyDeviceToHost));
    if (diff_out) HIPCHK(hipMemcpy(diff_out, ddiff, n * sizeof(float), hipMemcpyDeviceToHost));
    if (stats_out) HIPCHK(hipMemcpy(stats_out, dstats, 4 * sizeof(double), hipMemcpyDeviceToHost));
    return PDEIP_OK;
}

// Launches: 2 (pixels, final) with stats_out, 1 without.
extern "C" int pdeip_flow_crosscheck_dev(void *stream, const float *Uf, const float *Vf, const float *Ub, const float *Vb, int nrows, int ncols,
                                         double a, double b, float *mask_out, float *err_out, double *stats_out)
{
    const char *who = "pdeip_flow_crosscheck_dev";
    RC(flow_args(who, Uf, Vf, Ub, Vb, nrows, ncols, a, b, mask_out, err_out, stats_out));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid = pixel_grid(nrows, ncols, 1);
    double *partials = nullptr;
    int nparts = 0;
    if (stats_out != nullptr) RC(partials_for(grid, &partials, &nparts));
    hipLaunchKernelGGL(k_flow_crosscheck, grid, dim3(BLOCK), 0, s, Uf, Vf, Ub, Vb, nrows, ncols, a, b, mask_out, err_out, partials);
    if (stats_out != nullptr) hipLaunchKernelGGL(k_crosscheck_final, dim3(1), dim3(FINAL_BLOCK), 0, s, partials, nparts, stats_out);
    HIPCHK(hipGetLastError());
    tls.last_launches = stats_out != nullptr ? 2 : 1;
    return PDEIP_OK;
}

extern "C" int pdeip_flow_crosscheck(const float *Uf, const float *Vf, const float *Ub, const float *Vb, int nrows, int ncols, double a, double b,
                                     float *mask_out, float *err_out, double *stats_out)
{
    const char *who = "pdeip_flow_crosscheck";
    RC(flow_args(who, Uf, Vf, Ub, Vb, nrows, ncols, a, b, mask_out, err_out, stats_out));
    RC(use_device());
    const size_t n = (size_t)nrows * ncols, pn = pad4(n);
    // arena: the statistics (four doubles), then Uf, Vf, Ub, Vb, mask, err
    float *ar = nullptr;
    RC(ws_get(WS_ARENA, (8 + 6 * pn) * sizeof(float), &ar));
    double *dstats = stats_out ? reinterpret_cast<double *>(ar) : nullptr;
    float *in[4] = {ar + 8, ar + 8 + pn, ar + 8 + 2 * pn, ar + 8 + 3 * pn};
    const float *src[4] = {Uf, Vf, Ub, Vb};
    for (int k = 0; k < 4; k++) HIPCHK(hipMemcpy(in[k], src[k], n * sizeof(float), hipMemcpyHostToDevice));
    float *dmask = mask_out ? ar + 8 + 4 * pn : nullptr, *derr = err_out ? ar + 8 + 5 * pn : nullptr;
    RC(pdeip_flow_crosscheck_dev(nullptr, in[0], in[1], in[2], in[3], nrows, ncols, a, b, dmask, derr, dstats));
    if (mask_out) HIPCHK(hipMemcpy(mask_out, dmask, n * sizeof(float), hipMemcpyDeviceToHost));
    if (err_out) HIPCHK(hipMemcpy(err_out, derr, n * sizeof(float), hipMemcpyDeviceToHost));
    if (stats_out) HIPCHK(hipMemcpy(stats_out, dstats, 4 * sizeof(double), hipMemcpyDeviceToHost));
    return PDEIP_OK;
}
