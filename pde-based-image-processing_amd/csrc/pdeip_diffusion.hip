// pdeip_diffusion.hip -- libpdeip.so: Iout = Diffusion4_v10(I_in, 'alpha', alpha, 'outer_iter', K) (matlab/diffusion/
// Diffusion4_v10.m) as one resident call, pdeip_diffusion4 / pdeip_diffusion4_dev, before the driver's uint8 cast.
//
// Kernels: csrc/pdeip_diffusion.hpp (the line solve and its grid: csrc/pdeip_thomas.hpp).  The weights are k_diffweights6 (csrc/pdeip_pointwise.hpp, DdiffWeights) launched here
// directly: its entry point pdeip_diffweights6_dev keeps the gateway's 3x3 minimum, and this driver accepts 2-element lines.
// The maximum over the channels is the .m's max(w, [], 3), which omits a NaN of any channel (k_diffweights6<true>); the
// gateway's C keeps a NaN of its first frame (<false>, pdeip_diffweights6_dev).
// A Thomas solve has one order, so pdeip_set_mode does not apply.
//
// Build (build.py): hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -c, one object per translation unit.
#include "pdeip_ctx.hpp"
#include "pdeip_pointwise.hpp"
#include "pdeip_diffusion.hpp"

#include <cmath>

using namespace pdeip;
using namespace pdeip::diff;

namespace {

// Everything refused is refused here, before any HIP call.  NaN members (or no struct) keep the driver's defaults, alpha 25 and
// outer_iter 5 (Diffusion4_v10.m:36-37).  `for iter = 0:outer_iter` (:44) runs floor(outer_iter) + 1 iterations when
// outer_iter >= 0 and none below.  MATLAB's TDMA indexes d(0) on a line shorter than 2, so such images are refused.
// The column is blockIdx.y of k_diffweights6 and the channel blockIdx.y of k_diff4_lines: more than MAX_GRID_Y of either is
// the launch geometry's refusal (PDEIP_ERR_UNSUPPORTED), not the contract's.
constexpr int MAX_GRID_Y = 65535;

int diff4_args(const char *who, int nrows, int ncols, int channels, const pdeip_diffusion4_params *u, float *alpha, int *iters)
{
    if (nrows < 2 || ncols < 2)
        return set_err(PDEIP_ERR_ARG, "%s: image must be at least 2x2 (got %dx%d)", who, nrows, ncols);
    if (channels < 1) return set_err(PDEIP_ERR_ARG, "%s: number of channels must be >= 1 (got %d)", who, channels);
    if (ncols > MAX_GRID_Y) return set_err(PDEIP_ERR_UNSUPPORTED, "%s: more than %d columns (got %d)", who, MAX_GRID_Y, ncols);
    if (channels > MAX_GRID_Y) return set_err(PDEIP_ERR_UNSUPPORTED, "%s: more than %d channels (got %d)", who, MAX_GRID_Y, channels);
    if ((long long)nrows * ncols * channels > 0x7fffffffLL) return set_err(PDEIP_ERR_ARG, "%s: more than 2^31-1 elements", who);
    double a = 25.0, k = 5.0;
    if (u) {
        if (!std::isnan(u->alpha)) a = u->alpha;
        if (!std::isnan(u->outer_iter)) k = u->outer_iter;
    }
    if (!std::isfinite((float)a)) return set_err(PDEIP_ERR_ARG, "%s: alpha must be finite in single precision (got %g)", who, a);
    if (std::isinf(k)) return set_err(PDEIP_ERR_ARG, "%s: outer_iter must be finite (got %g)", who, k);
    if (k > 2147483646.0) return set_err(PDEIP_ERR_ARG, "%s: outer_iter = %g is too large", who, k);
    *alpha = (float)a; // the double parameter meets single arrays
    *iters = k >= 0.0 ? (int)std::floor(k) + 1 : 0;
    return PDEIP_OK;
}

} // namespace

// The run: Iout = single(I_in), then per outer iteration the weights of Iout (maximum over the channels, NaN omitted), the
// column and row solves of every channel, Iout = ver + hor.  Workspace (WS_DRIVER): the four [nrows x ncols] weight planes
// (k_diffweights6 writes frame 0 only), then xc, xr and the column and row cp/dp, [nrows x ncols x channels] each.
extern "C" int pdeip_diffusion4_dev(void *stream, const float *Iin, int nrows, int ncols, int channels,
                                    const pdeip_diffusion4_params *prm, float *Iout)
{
    const char *who = "pdeip_diffusion4_dev";
    NONNULL(who, Iin); NONNULL(who, Iout);
    float alpha = 0.0f;
    int iters = 0;
    RC(diff4_args(who, nrows, ncols, channels, prm, &alpha, &iters));
    const size_t n = (size_t)nrows * ncols, nc = n * channels, pn = pad4(n), pc = pad4(nc);
    hipStream_t s = static_cast<hipStream_t>(stream);
    int launches = 0;
    if (Iout != Iin) {
        RC(copy_d2d(s, Iout, Iin, nc));
        launches++;
    }
    if (iters > 0) {
        float *ws = nullptr;
        RC(ws_get(WS_DRIVER, (4 * pn + 6 * pc) * sizeof(float), &ws));
        float *wW = ws, *wN = wW + pn, *wE = wN + pn, *wS = wE + pn;
        const thomas::Planes w = thomas::carve_planes(wS + pn, pc);
        const dim3 lines = thomas::lines_grid(nrows, ncols, channels), sum((unsigned)((nc + 255) / 256));
        for (int it = 0; it < iters; it++) {
            hipLaunchKernelGGL(k_diffweights6<true>, pixel_grid(nrows, ncols, 1), dim3(256), 0, s, wW, wN, wE, wS, Iout, nrows, ncols,
                               channels, 0.00001f);
            hipLaunchKernelGGL(k_diff4_lines, lines, dim3(thomas::BLOCK), 0, s, Iout, wW, wN, wE, wS, w.xc, w.xr, w.cpc, w.dpc, w.cpr,
                               w.dpr, nrows, ncols, thomas::line_blocks(nrows), alpha);
            hipLaunchKernelGGL(k_diff4_combine, sum, dim3(256), 0, s, w.xc, w.xr, Iout, nc);
            HIPCHK(hipGetLastError());
            launches += 3;
        }
    }
    tls.last_launches = launches;
    return PDEIP_OK;
}

extern "C" int pdeip_diffusion4(const float *Iin, int nrows, int ncols, int channels, const pdeip_diffusion4_params *prm, float *Iout)
{
    const char *who = "Diffusion4_v10";
    NONNULL(who, Iin); NONNULL(who, Iout);
    float alpha = 0.0f;
    int iters = 0;
    RC(diff4_args(who, nrows, ncols, channels, prm, &alpha, &iters));
    RC(use_device());
    const size_t nc = (size_t)nrows * ncols * channels;
    float *dI = nullptr;
    RC(ws_get(WS_ARENA, pad4(nc) * sizeof(float), &dI));
    HIPCHK(hipMemcpy(dI, Iin, nc * sizeof(float), hipMemcpyHostToDevice));
    RC(pdeip_diffusion4_dev(nullptr, dI, nrows, ncols, channels, prm, dI));
    HIPCHK(hipMemcpy(Iout, dI, nc * sizeof(float), hipMemcpyDeviceToHost));
    return PDEIP_OK;
}
