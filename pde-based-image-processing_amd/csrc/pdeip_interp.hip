// pdeip_interp.hip -- libpdeip.so: the frame between two frames, from a computed flow.
//
//   the flow of frame 0 -> 1 carried forward to time t, conflicts settled by cost then index   pdeip_flow_splat_dev
//   both frames sampled along the flow at t and blended, occlusions decided by the masks       pdeip_interp_blend_dev
//   cross-checks, splat, hole filling and blend as one resident chain                           pdeip_flow_interpolate(_dev)
//
// Kernels: csrc/pdeip_interp.hpp; the contract: include/pdeip.h.  The splat and the blend have no ordering; the chain's hole filling
// runs pdeip_tv_inpaint4_dev in the library's current mode.  Nothing is read back in the _dev forms and no launch depends on the data.
//
// Build (build.py): hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -c, one object per translation unit.
#include "pdeip_ctx.hpp"
#include "pdeip_interp.hpp"

#include <cmath>

using namespace pdeip;
using namespace pdeip::interp;

namespace {

constexpr int MAX_GRID_Y = 65535; // the column is blockIdx.y
constexpr int SPLAT_LAUNCHES = 3, BLEND_LAUNCHES = 1;

int shape_args(const char *who, int nrows, int ncols)
{
    if (nrows < 3 || ncols < 3) return set_err(PDEIP_ERR_ARG, "%s: the field must be at least 3x3 (got %dx%d)", who, nrows, ncols);
    if ((long long)nrows * ncols > 0x7fffffffLL) return set_err(PDEIP_ERR_ARG, "%s: more than 2^31-1 pixels", who);
    if (ncols > MAX_GRID_Y) return set_err(PDEIP_ERR_UNSUPPORTED, "%s: more than %d columns (got %d)", who, MAX_GRID_Y, ncols);
    return PDEIP_OK;
}

int time_arg(const char *who, double t)
{
    if (!(t > 0.0 && t < 1.0)) return set_err(PDEIP_ERR_ARG, "%s: t must lie strictly between 0 and 1 (got %g)", who, t);
    return PDEIP_OK;
}

int pair_arg(const char *who, const char *a_name, const void *a, const char *b_name, const void *b)
{
    if ((a != nullptr) != (b != nullptr)) return set_err(PDEIP_ERR_ARG, "%s: %s and %s must both be given or both be NULL", who, a_name, b_name);
    return PDEIP_OK;
}

int channels_arg(const char *who, int channels)
{
    if (channels < 1) return set_err(PDEIP_ERR_ARG, "%s: channels must be >= 1 (got %d)", who, channels);
    return PDEIP_OK;
}

struct Named {
    const char *name;
    const void *p;
};

template <int NO, int NI>
int alias_args(const char *who, const Named (&outs)[NO], const Named (&ins)[NI])
{
    for (const Named &o : outs)
        for (const Named &in : ins)
            if (o.p != nullptr && o.p == in.p) return set_err(PDEIP_ERR_ARG, "%s: the output %s is the input %s", who, o.name, in.name);
    return PDEIP_OK;
}

// Everything refused is refused here, before any HIP call.
int splat_args(const char *who, const void *Uf, const void *Vf, const void *I0, const void *I1, int channels, int nrows, int ncols, double t,
               const void *Ut_out, const void *Vt_out, const void *cost_out)
{
    NONNULL(who, Uf); NONNULL(who, Vf); NONNULL(who, Ut_out); NONNULL(who, Vt_out);
    RC(pair_arg(who, "I0", I0, "I1", I1));
    if (I0 != nullptr) RC(channels_arg(who, channels));
    RC(time_arg(who, t));
    RC(shape_args(who, nrows, ncols));
    const Named outs[3] = {{"Ut_out", Ut_out}, {"Vt_out", Vt_out}, {"cost_out", cost_out}};
    const Named ins[4] = {{"Uf", Uf}, {"Vf", Vf}, {"I0", I0}, {"I1", I1}};
    return alias_args(who, outs, ins);
}

int blend_args(const char *who, const void *I0, const void *I1, int channels, const void *Ut, const void *Vt, const void *M0, const void *M1,
               int nrows, int ncols, double t, const void *It_out, const void *source_out)
{
    NONNULL(who, I0); NONNULL(who, I1); NONNULL(who, Ut); NONNULL(who, Vt); NONNULL(who, It_out);
    RC(channels_arg(who, channels));
    RC(pair_arg(who, "M0", M0, "M1", M1));
    RC(time_arg(who, t));
    RC(shape_args(who, nrows, ncols));
    const Named outs[2] = {{"It_out", It_out}, {"source_out", source_out}};
    const Named ins[6] = {{"I0", I0}, {"I1", I1}, {"Ut", Ut}, {"Vt", Vt}, {"M0", M0}, {"M1", M1}};
    return alias_args(who, outs, ins);
}

// The chain's parameters with the defaults filled in.
struct Resolved {
    double a, b;
    int use_costs;
    const pdeip_inpaint_params *fill;
};

int chain_args(const char *who, const void *I0, const void *I1, int channels, const void *Uf, const void *Vf, const void *Ub, const void *Vb,
               int nrows, int ncols, double t, const pdeip_interp_params *prm, const void *It_out, const void *Ut_out, const void *Vt_out,
               const void *source_out, Resolved *p)
{
    NONNULL(who, I0); NONNULL(who, I1); NONNULL(who, Uf); NONNULL(who, Vf); NONNULL(who, It_out);
    RC(channels_arg(who, channels));
    RC(pair_arg(who, "Ub", Ub, "Vb", Vb));
    RC(time_arg(who, t));
    RC(shape_args(who, nrows, ncols));
    *p = Resolved{0.01, 0.5, 1, nullptr};
    if (prm != nullptr) *p = Resolved{prm->a, prm->b, prm->use_costs != 0, prm->fill};
    if (!(p->a >= 0.0) || !(p->b >= 0.0)) return set_err(PDEIP_ERR_ARG, "%s: a and b must be >= 0 and not NaN (got %g, %g)", who, p->a, p->b);
    RC(inpaint_check_params(who, nrows, ncols, 2, p->fill));
    const Named outs[4] = {{"It_out", It_out}, {"Ut_out", Ut_out}, {"Vt_out", Vt_out}, {"source_out", source_out}};
    const Named ins[6] = {{"I0", I0}, {"I1", I1}, {"Uf", Uf}, {"Vf", Vf}, {"Ub", Ub}, {"Vb", Vb}};
    return alias_args(who, outs, ins);
}

// The chain's scratch, in floats: the two masks, the splatted flow [nrows x ncols x 2] and the filled one.
size_t chain_scratch(size_t n) { return 2 * pad4(n) + 2 * pad4(2 * n); }

// Cross-checks, splat, fill, blend on s.  scratch: chain_scratch(n) floats of device memory.
int run_chain(hipStream_t s, const float *I0, const float *I1, int channels, const float *Uf, const float *Vf, const float *Ub, const float *Vb,
              int nrows, int ncols, double t, const Resolved &p, float *scratch, float *It_out, float *Ut_out, float *Vt_out, float *source_out)
{
    const size_t n = (size_t)nrows * ncols;
    float *M0 = scratch, *M1 = M0 + pad4(n), *S = M1 + pad4(n), *F = S + pad4(2 * n);
    int launches = 0, expected = SPLAT_LAUNCHES + BLEND_LAUNCHES;
    if (Ub != nullptr) {
        RC(pdeip_flow_crosscheck_dev(s, Uf, Vf, Ub, Vb, nrows, ncols, p.a, p.b, M0, nullptr, nullptr));
        launches += tls.last_launches;
        RC(pdeip_flow_crosscheck_dev(s, Ub, Vb, Uf, Vf, nrows, ncols, p.a, p.b, M1, nullptr, nullptr));
        launches += tls.last_launches;
        expected += 2;
    }
    const bool costs = p.use_costs != 0;
    RC(pdeip_flow_splat_dev(s, Uf, Vf, costs ? I0 : nullptr, costs ? I1 : nullptr, channels, nrows, ncols, t, S, S + n, nullptr));
    launches += tls.last_launches;
    RC(pdeip_tv_inpaint4_dev(s, S, nrows, ncols, 2, nullptr, 0, p.fill, F, nullptr));
    launches += tls.last_launches;
    expected += tls.last_launches;
    const bool masks = Ub != nullptr;
    RC(pdeip_interp_blend_dev(s, I0, I1, channels, F, F + n, masks ? M0 : nullptr, masks ? M1 : nullptr, nrows, ncols, t, It_out, source_out));
    launches += tls.last_launches;
    if (Ut_out != nullptr) {
        RC(copy_d2d(s, Ut_out, F, n));
        launches++;
        expected++;
    }
    if (Vt_out != nullptr) {
        RC(copy_d2d(s, Vt_out, F + n, n));
        launches++;
        expected++;
    }
    if (launches != expected) return set_err(PDEIP_ERR_DEVICE, "pdeip_flow_interpolate: %d launches where the parts sum to %d", launches, expected);
    tls.last_launches = launches;
    return PDEIP_OK;
}

} // namespace

// Launches: 3 (clear, splat, resolve), whatever the data.
extern "C" int pdeip_flow_splat_dev(void *stream, const float *Uf, const float *Vf, const float *I0, const float *I1, int channels, int nrows,
                                    int ncols, double t, float *Ut_out, float *Vt_out, float *cost_out)
{
    const char *who = "pdeip_flow_splat_dev";
    RC(splat_args(who, Uf, Vf, I0, I1, channels, nrows, ncols, t, Ut_out, Vt_out, cost_out));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t n = (size_t)nrows * ncols;
    float *ws = nullptr;
    RC(ws_get(WS_INTERP, n * sizeof(unsigned long long), &ws)); // hipMalloc'ed: aligned far beyond 8 bytes
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(ws);
    const dim3 grid = pixel_grid(nrows, ncols, 1);
    size_t blocks = (n + BLOCK - 1) / BLOCK;
    if (blocks > 256 * 16) blocks = 256 * 16; // grid-stride beyond 16 workgroups per compute unit
    int launches = 0;
    hipLaunchKernelGGL(k_splat_clear, dim3((unsigned)blocks), dim3(BLOCK), 0, s, keys, n);
    launches++;
    hipLaunchKernelGGL(k_flow_splat, grid, dim3(BLOCK), 0, s, Uf, Vf, I0, I1, channels, nrows, ncols, t, keys);
    launches++;
    hipLaunchKernelGGL(k_splat_resolve, grid, dim3(BLOCK), 0, s, keys, Uf, Vf, nrows, ncols, Ut_out, Vt_out, cost_out);
    launches++;
    HIPCHK(hipGetLastError());
    if (launches != SPLAT_LAUNCHES) return set_err(PDEIP_ERR_DEVICE, "%s: %d launches where %d are stated", who, launches, SPLAT_LAUNCHES);
    tls.last_launches = launches;
    return PDEIP_OK;
}

// Launches: 1.
extern "C" int pdeip_interp_blend_dev(void *stream, const float *I0, const float *I1, int channels, const float *Ut, const float *Vt,
                                      const float *M0, const float *M1, int nrows, int ncols, double t, float *It_out, float *source_out)
{
    const char *who = "pdeip_interp_blend_dev";
    RC(blend_args(who, I0, I1, channels, Ut, Vt, M0, M1, nrows, ncols, t, It_out, source_out));
    const double tq = 1.0 - t;
    hipLaunchKernelGGL(k_interp_blend, pixel_grid(nrows, ncols, 1), dim3(BLOCK), 0, static_cast<hipStream_t>(stream), I0, I1, channels, Ut, Vt, M0,
                       M1, nrows, ncols, t, tq, It_out, source_out);
    HIPCHK(hipGetLastError());
    tls.last_launches = BLEND_LAUNCHES;
    return PDEIP_OK;
}

// Launches: [2 with Ub, Vb] + 3 + pdeip_tv_inpaint4_dev's on two frames without a guide + 1 + one per Ut_out / Vt_out given.
// Scratch (WS_ARENA): chain_scratch().
extern "C" int pdeip_flow_interpolate_dev(void *stream, const float *I0, const float *I1, int channels, const float *Uf, const float *Vf,
                                          const float *Ub, const float *Vb, int nrows, int ncols, double t, const pdeip_interp_params *prm,
                                          float *It_out, float *Ut_out, float *Vt_out, float *source_out)
{
    const char *who = "pdeip_flow_interpolate_dev";
    Resolved p;
    RC(chain_args(who, I0, I1, channels, Uf, Vf, Ub, Vb, nrows, ncols, t, prm, It_out, Ut_out, Vt_out, source_out, &p));
    float *scratch = nullptr;
    RC(ws_get(WS_ARENA, chain_scratch((size_t)nrows * ncols) * sizeof(float), &scratch));
    return run_chain(static_cast<hipStream_t>(stream), I0, I1, channels, Uf, Vf, Ub, Vb, nrows, ncols, t, p, scratch, It_out, Ut_out, Vt_out,
                     source_out);
}

extern "C" int pdeip_flow_interpolate(const float *I0, const float *I1, int channels, const float *Uf, const float *Vf, const float *Ub,
                                      const float *Vb, int nrows, int ncols, double t, const pdeip_interp_params *prm, float *It_out,
                                      float *Ut_out, float *Vt_out, float *source_out)
{
    const char *who = "pdeip_flow_interpolate";
    Resolved p;
    RC(chain_args(who, I0, I1, channels, Uf, Vf, Ub, Vb, nrows, ncols, t, prm, It_out, Ut_out, Vt_out, source_out, &p));
    RC(use_device());
    const size_t n = (size_t)nrows * ncols, pn = pad4(n), pc = pad4(n * channels);
    // arena: the chain's scratch, then I0, I1, It, then Uf, Vf, Ub, Vb, Ut, Vt, source
    float *ar = nullptr;
    RC(ws_get(WS_ARENA, (chain_scratch(n) + 3 * pc + 7 * pn) * sizeof(float), &ar));
    float *dI0 = ar + chain_scratch(n), *dI1 = dI0 + pc, *dIt = dI1 + pc, *dUf = dIt + pc, *dVf = dUf + pn;
    float *dUb = Ub ? dVf + pn : nullptr, *dVb = Ub ? dVf + 2 * pn : nullptr;
    float *dUt = Ut_out ? dVf + 3 * pn : nullptr, *dVt = Vt_out ? dVf + 4 * pn : nullptr, *dsrc = source_out ? dVf + 5 * pn : nullptr;
    HIPCHK(hipMemcpy(dI0, I0, n * channels * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dI1, I1, n * channels * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dUf, Uf, n * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dVf, Vf, n * sizeof(float), hipMemcpyHostToDevice));
    if (Ub) {
        HIPCHK(hipMemcpy(dUb, Ub, n * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(dVb, Vb, n * sizeof(float), hipMemcpyHostToDevice));
    }
    RC(run_chain(nullptr, dI0, dI1, channels, dUf, dVf, dUb, dVb, nrows, ncols, t, p, ar, dIt, dUt, dVt, dsrc));
    HIPCHK(hipMemcpy(It_out, dIt, n * channels * sizeof(float), hipMemcpyDeviceToHost));
    if (Ut_out) HIPCHK(hipMemcpy(Ut_out, dUt, n * sizeof(float), hipMemcpyDeviceToHost));
    if (Vt_out) HIPCHK(hipMemcpy(Vt_out, dVt, n * sizeof(float), hipMemcpyDeviceToHost));
    if (source_out) HIPCHK(hipMemcpy(source_out, dsrc, n * sizeof(float), hipMemcpyDeviceToHost));
    RC(pdeip_persist_error());
    return PDEIP_OK;
}
