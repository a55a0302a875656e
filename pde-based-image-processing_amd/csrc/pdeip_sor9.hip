// pdeip_sor9.hip -- libpdeip.so: point SOR, 9-point model (PDEsolver8): launch logic and the *_dev entry point.
//
// Build (build.py): hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -c, one object per translation unit.
// -ffp-contract=off is part of the parity contract: the reference is plain C built without FMA.
#include "pdeip_ctx.hpp"

#include "pdeip_models.hpp"
#include "pdeip_pointwise.hpp"
#include "pdeip_sor_pde8.hpp"
#include "pdeip_sor_pde8_persist.hpp"
#include "pdeip_persist_host.hpp"
#include "pdeip_sor_rb.hpp"
#include "pdeip_sor_plan.hpp"

using namespace pdeip;

namespace {

static_assert(P8_R == EX_R && P8_G == P8_SKEW + 1 && P8_H == P8_SKEW + 2, "plan_exact's fronts");
const SorTraits PDE8_TRAITS{1, ModelPde8::NCF, true, P8_SKEW, P8_OWN_ROWS2, false, 1, 1, 0, nullptr, nullptr};

// The four-colour kernels by (two sweeps, vector accesses, first launch of the call).
auto p8_kernel(bool two, bool vec, bool first)
{
    static constexpr decltype(&k_pde8_colour<true, true>) table[2][2][2] = {
        {{&k_pde8_colour<false, false>, &k_pde8_colour<false, true>}, {&k_pde8_colour<true, false>, &k_pde8_colour<true, true>}},
        {{&k_pde8_colour2<false, false>, &k_pde8_colour2<false, true>}, {&k_pde8_colour2<true, false>, &k_pde8_colour2<true, true>}}};
    return table[two][vec][first];
}

// A call, as the runners see it.  cf: the RAW planes in the two derived slots (B, TRACE), then the eight weights; bt / inv: the
// workspace planes B_temp / INV_TRACE are built into.
struct Pde8Call {
    hipStream_t s;
    float *X;
    const float *cf[ModelPde8::NCF];
    float *bt, *inv;
    int nrows, ncols, nframes, iter;
    float omega;
    int col0;
    size_t n; // pixels of a frame
};

// Exact order: one launch per call (progress counters) or one per front, then the border replicate.
int run_exact(const Pde8Call &c, const SorPlan &plan)
{
    const float *const *w = c.cf;
    hipStream_t s = c.s;
    Pde8Planes P{};
    P.x = c.X;
    for (int f = 0; f < ModelPde8::NCF; f++) P.cf[f] = f == ModelPde8::cB ? c.bt : (f == ModelPde8::cInv ? c.inv : w[f]);
    float *scratch = nullptr;
    RC(ws_get(WS_PING, pde8_exact_scratch_floats(c.nrows, c.ncols, c.nframes, c.iter) * sizeof(float), &scratch));
    int nl;
    if (plan.form == FORM_PERSIST) {
        // pre-pass: B_temp / INV_TRACE and the eight weights of a pixel side by side (k_pde8_pack)
        float *pack = nullptr;
        RC(ws_get(WS_PACK, pde8_pack_floats(c.nrows, c.ncols, c.nframes) * sizeof(float), &pack));
        hipLaunchKernelGGL(k_pde8_pack, dim3((unsigned)((pde8_pack_blocks(c.nrows) + 127) / 128), (unsigned)c.ncols, (unsigned)c.nframes), dim3(128), 0, s, pack, w[1], w[0],
                           w[2], w[3], w[4], w[5], w[6], w[7], w[8], w[9], c.nrows, c.ncols, c.n);
        // schedule table, control block, mailbox: one 8-byte {value, tag} word per (frame, sweep, strip, step of the walk)
        PersistCtl ctl{};
        RC(persist_prepare(s, plan.B, c.iter, c.nframes, (size_t)c.nframes * c.iter * plan.B * (size_t)plan.NC * EX_CH * sizeof(unsigned long long), &ctl));
        SweepTimer timer(s);
        nl = pde8_run_exact_persist(s, P, pack, scratch, ctl, c.nrows, c.ncols, c.nframes, c.iter, c.omega);
        if (nl >= 0) timer.stop(1);
    } else {
        hipLaunchKernelGGL(k_pde8_divisors, pixel_grid(c.nrows, c.ncols, c.nframes), dim3(256), 0, s, c.bt, c.inv, w[1], w[0], w[2], w[3], w[4], w[5], w[6], w[7], w[8],
                           w[9], c.nrows, c.ncols, c.n);
        SweepTimer timer(s);
        nl = pde8_run_exact(s, P, scratch, c.nrows, c.ncols, c.nframes, c.iter, c.omega);
        if (nl >= 0) timer.stop(nl);
    }
    if (nl < 0) return PDEIP_ERR_DEVICE; // LDS opt-in refused (message set by ensure_lds)
    tls.last_launches += 1 + nl;
    HIPCHK(hipGetLastError());
    return PDEIP_OK;
}

// Four-colour: fused launches that ping-pong with a scratch copy; the first builds B_temp / INV_TRACE.
int run_chain(const Pde8Call &c, const SorPlan &plan)
{
    const size_t nf = c.n * (size_t)c.nframes;
    float *buf[2] = {c.X, nullptr};
    RC(ws_get(WS_PING, nf * sizeof(float), &buf[BUF_SCRATCH]));
    Pde8SweepPlanes P{};
    for (int f = 0; f < ModelPde8::NCF; f++) P.cf[f] = c.cf[f];
    SweepTimer timer(c.s);
    RC(for_each_launch(plan, [&](const SorLaunch &l) {
        P.x_in = buf[l.src];
        P.x_out = buf[l.dst];
        hipLaunchKernelGGL(p8_kernel(l.sweeps == 2, plan.vec, l.first), dim3((unsigned)l.gridx, (unsigned)c.nframes), dim3(64 * RB_WAVES_PER_BLOCK), 0, c.s, P,
                           l.first ? c.bt : nullptr, l.first ? c.inv : nullptr, c.nrows, c.ncols, l.tj, l.tiles, l.units, c.omega, c.col0, c.n);
        if (l.first) {
            P.cf[ModelPde8::cB] = c.bt;
            P.cf[ModelPde8::cInv] = c.inv;
        }
        tls.last_launches++;
        return PDEIP_OK;
    }));
    timer.stop(plan.nlaunch);
    if (plan.copy_back) RC(copy_d2d(c.s, c.X, buf[BUF_SCRATCH], nf));
    HIPCHK(hipGetLastError());
    return PDEIP_OK;
}

} // namespace

SorPlan pdeip::plan_sor_pde8(SorShape sh, const SorDevice &dev)
{
    sh.has_dst = false; // the entry point has no destination
    sh.packed_frame_bytes = pde8_pack_floats(sh.nrows, sh.ncols, 1) * sizeof(float);
    sh.persist_chunks = pde8_persist_chunks(sh.nrows);
    // the only fact the four-colour chain asks: resident waves of the fused kernel (see pick_rb2_tj)
    return plan_sor(PDE8_TRAITS, sh, dev, [](int) { return resident_waves(reinterpret_cast<const void *>(p8_kernel(true, true, false)), 64 * RB_WAVES_PER_BLOCK, RB_WAVES_PER_BLOCK); });
}

extern "C" int pdeip_pde_sor8_dev(void *stream, float *X, const float *TRACE, const float *B, const float *wW,
                                  const float *wNW, const float *wN, const float *wNE, const float *wE,
                                  const float *wSE, const float *wS, const float *wSW, int nrows, int ncols,
                                  int nframes, int iter, float omega, int mode, int col0)
{
    const char *who = "pdeip_pde_sor8_dev";
    RC(check_dims(who, nrows, ncols, nframes));
    RC(check_mode(who, mode));
    tls.last_launches = 0;
    tls.last_directions.clear(); // the nine-point kernels have no mirrored march
    Pde8Call c{static_cast<hipStream_t>(stream), X, {B, TRACE, wW, wNW, wN, wNE, wE, wSE, wS, wSW}, nullptr, nullptr, nrows, ncols, nframes, iter, omega, col0,
               (size_t)nrows * ncols};
    bool aligned = aligned16(X);
    for (int f = 0; f < ModelPde8::NCF; f++) aligned = aligned && aligned16(c.cf[f]);
    const SorPlan plan = plan_sor_pde8(SorShape{nrows, ncols, nframes, iter, mode, aligned, false, 0, 0}, SorDevice{});
    if (plan.family == SOR_NONE) return PDEIP_OK;
    RC(ws_get(WS_AUX0, c.n * nframes * sizeof(float), &c.bt));
    RC(ws_get(WS_AUX1, c.n * nframes * sizeof(float), &c.inv));
    return plan.family == SOR_EXACT ? run_exact(c, plan) : run_chain(c, plan);
}

#ifdef PDEIP_P8_STAMPS
extern "C" int pdeip_debug_read_p8_stamps(unsigned long long *out)
{
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_p8_stamps), 4096 * sizeof(unsigned long long)));
    return PDEIP_OK;
}
#endif
