// pdeip_sor5.hip -- libpdeip.so: point SOR, 5-point models: launch logic (red-black / exact order) and the *_dev entry points.
//
// Build (build.py): hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -c, one object per translation unit.
// -ffp-contract=off is part of the parity contract: the reference is plain C built without FMA.
#include "pdeip_ctx.hpp"

#include "pdeip_models.hpp"
#include "pdeip_pointwise.hpp"
#include "pdeip_sor_exact.hpp"
#include "pdeip_walk_host.hpp"
#include "pdeip_persist_host.hpp"
#include "pdeip_sor_rb.hpp"
#include "pdeip_sor_rbp.hpp"
#include "pdeip_sor_small.hpp"
#include "pdeip_sor_plan.hpp"

using namespace pdeip;

namespace {

constexpr int PS = RBP_SWEEPS;

template <class Mdl> SorTraits sor_traits()
{
    using PL = RbpLayout<Mdl, PS>;
    return SorTraits{Mdl::NIT, Mdl::NCF, false, 1, RB_OWN_ROWS, PL::FITS, PL::NW, RBP_OWN_ROWS, PL::nsteps(0), &SmallLayout<Mdl>::plan, &walk_width<Mdl>};
}

// The kernels of the red-black chain by (vector accesses, first launch of the call, two sweeps).
template <class Mdl> auto rb_kernel(bool vec, bool first, bool two)
{
    static constexpr decltype(&k_sor_rb<Mdl, true, true, true>) table[2][2][2] = {
        {{&k_sor_rb<Mdl, false, false, false>, &k_sor_rb<Mdl, false, false, true>}, {&k_sor_rb<Mdl, false, true, false>, &k_sor_rb<Mdl, false, true, true>}},
        {{&k_sor_rb<Mdl, true, false, false>, &k_sor_rb<Mdl, true, false, true>}, {&k_sor_rb<Mdl, true, true, false>, &k_sor_rb<Mdl, true, true, true>}}};
    return table[vec][first][two];
}
template <class Mdl> auto rbp_kernel(bool first) { return first ? &k_sor_rbp<Mdl, PS, true> : &k_sor_rbp<Mdl, PS, false>; }

// A device fact the planner was not given, asked from the current device (cached per device).  Both instantiations of k_sor_rbp
// take the same LDS, more than half of a compute unit's: one workgroup per compute unit either way, so one of them is asked.
template <class Mdl> int device_fact(int fact)
{
    using PL = RbpLayout<Mdl, PS>;
    if (fact == FACT_CUS) return device_cus() > 0 ? device_cus() : 1;
    if (fact == FACT_RB2) return resident_waves(reinterpret_cast<const void *>(rb_kernel<Mdl>(true, false, true)), 64 * RB_WAVES_PER_BLOCK, RB_WAVES_PER_BLOCK);
    return resident_waves(reinterpret_cast<const void *>(rbp_kernel<Mdl>(true)), PL::THREADS, 1, PL::LDS_BYTES);
}

template <class Mdl> SorPlan plan_for(const SorShape &sh, const SorDevice &dev) { return plan_sor(sor_traits<Mdl>(), sh, dev, &device_fact<Mdl>); }

// ------------------------------------------------------------------------------------------------
// sweep drivers (5-point models)
// ------------------------------------------------------------------------------------------------

// A call, as the runners see it.  P.it_out holds the caller's iterate, P.ro and P.cf are set, with the RAW planes in the two
// derived slots (Mdl::D0, Mdl::D1); aux0 / aux1 are the workspace planes the derived ones (divisors) are built into.
template <class Mdl> struct SweepCall {
    hipStream_t s;
    SweepPlanes<Mdl> P;
    int nrows, ncols, nframes, iter;
    float omega;
    int col0;
    size_t n; // pixels of a frame
    float *aux0, *aux1;
    float *const *dst;
};

// Exact order: the wavefront kernels relax in place, on the destination when there is one (run_sweeps copied the iterate there).
template <class Mdl> int run_exact(const SweepCall<Mdl> &c, const SorPlan &plan)
{
    constexpr int NIT = Mdl::NIT;
    SweepPlanes<Mdl> P = c.P;
    hipStream_t s = c.s;
    for (int f = 0; f < NIT; f++) {
        if (c.dst) P.it_out[f] = c.dst[f];
        P.it_in[f] = P.it_out[f];
    }
    if (plan.form == FORM_FRONT) {
        hipLaunchKernelGGL(k_derive<Mdl>, pixel_grid(c.nrows, c.ncols, c.nframes), dim3(256), 0, s, P, c.aux0, c.aux1, c.nrows, c.ncols, c.n);
        P.cf[Mdl::D0] = c.aux0;
        P.cf[Mdl::D1] = c.aux1;
        const dim3 grid((unsigned)(plan.B * c.iter), (unsigned)c.nframes);
        constexpr size_t lds = ExactLayout<Mdl>::LDS_BYTES;
        RC(ensure_lds(reinterpret_cast<const void *>(&k_sor_exact<Mdl>), lds)); // > 64 KiB of dynamic LDS needs an explicit opt-in
        SweepTimer timer(s);
        for (int m = 0; m <= plan.last_m; m++)
            hipLaunchKernelGGL(k_sor_exact<Mdl>, grid, dim3(128), lds, s, P, c.nrows, c.ncols, plan.A, plan.B, c.iter, m, c.omega, c.n);
        timer.stop(plan.last_m + 1);
        tls.last_launches += 1 + plan.last_m + 1;
    } else {
        // pre-pass of the persistent forms: the derived planes AND the raw ones, packed per pixel (k_pack_coefficients)
        float *pack = nullptr;
        RC(ws_get(WS_PACK, c.n * c.nframes * Mdl::NCF * sizeof(float), &pack));
        hipLaunchKernelGGL(k_pack_coefficients<Mdl>, pixel_grid(c.nrows, c.ncols, c.nframes), dim3(256), 0, s, P, pack, c.nrows, c.ncols, c.n);
        // schedule table, control block, mailbox: one 8-byte {value, tag} word per (frame, sweep, strip, field, row)
        PersistCtl ctl{};
        RC(persist_prepare(s, plan.B, c.iter, c.nframes, (size_t)c.nframes * c.iter * plan.B * NIT * (size_t)plan.NC * EX_CH * sizeof(unsigned long long), &ctl));
        SweepTimer timer(s);
        if (plan.form == FORM_WALK) {
            RC(walk_launch<Mdl>(s, P, pack, ctl, c.nrows, c.ncols, plan.B, c.iter, plan.NC, c.nframes, c.omega, c.n, plan.W));
        } else { // one launch, progress counters instead of one launch per front
            constexpr size_t plds = ExactLayout<Mdl>::LDS_BYTES + 16;
            RC(ensure_lds(reinterpret_cast<const void *>(&k_sor_exact_persist<Mdl>), plds));
            hipLaunchKernelGGL(k_sor_exact_persist<Mdl>, dim3((unsigned)(plan.B * c.iter * c.nframes)), dim3(exp_threads<Mdl>()), plds, s, P, pack, ctl, c.nrows,
                               c.ncols, plan.B, c.iter, plan.NC, c.nframes, c.omega, c.n);
        }
        timer.stop(1);
        tls.last_launches += 2;
    }
    const int nb = 2 * c.ncols + 2 * (c.nrows - 2);
    hipLaunchKernelGGL(k_fill_borders, dim3((nb + 255) / 256, c.nframes, NIT), dim3(256), 0, s, P.it_out[0], P.it_out[NIT - 1], NIT, c.nrows, c.ncols, c.n);
    tls.last_launches++;
    HIPCHK(hipGetLastError());
    return PDEIP_OK;
}

// The buffers a launch reads and writes: buf[BUF_*][field].
template <class Mdl> void bind_buffers(SweepPlanes<Mdl> &P, float *(&buf)[3][Mdl::NIT], const SorLaunch &l)
{
    for (int f = 0; f < Mdl::NIT; f++) {
        P.it_in[f] = buf[l.src][f];
        P.it_out[f] = buf[l.dst][f];
    }
}

// k_sor_small: later launches of the call run in place on the result.
template <class Mdl> int run_small(const SweepCall<Mdl> &c, const SorPlan &plan, float *(&buf)[3][Mdl::NIT])
{
    using SL = SmallLayout<Mdl>;
    const SmallPlan &sp = plan.small;
    SweepPlanes<Mdl> P = c.P;
    RC(ensure_lds(reinterpret_cast<const void *>(&k_sor_small<Mdl>), sp.lds));
    unsigned *counter = nullptr, *abort_word = nullptr;
    if (sp.nslabs > 1) {
        float *p = nullptr;
        RC(ws_get(WS_SMALL, 64, &p));
        counter = reinterpret_cast<unsigned *>(p);
        RC(ws_get(WS_CTL, 16, &p));
        abort_word = reinterpret_cast<unsigned *>(p);
    }
    DeviceState *d = cur_dev();
    SweepTimer timer(c.s);
    RC(for_each_launch(plan, [&](const SorLaunch &l) {
        bind_buffers<Mdl>(P, buf, l);
        const bool gated = sp.nslabs > 1 && l.src == l.dst; // a cut frame relaxed in place: the load counter
        if (gated) d->persist_used = true; // a timed-out wait raises the sticky abort word
        hipLaunchKernelGGL(k_sor_small<Mdl>, dim3((unsigned)sp.nslabs, (unsigned)c.nframes), dim3(SL::THREADS), sp.lds, c.s, P, c.nrows, c.ncols, l.sweeps,
                           c.omega, c.col0, c.n, sp.W, gated ? counter : nullptr, abort_word);
        tls.last_launches++;
        return PDEIP_OK;
    }));
    timer.stop(plan.nlaunch);
    HIPCHK(hipGetLastError());
    return PDEIP_OK;
}

#ifndef PDEIP_TIMER_MARKERS
#define PDEIP_TIMER_MARKERS 0 /* A/B aid: record the two events as markers around the chain, as every other path does */
#endif

// The red-black chain.  In place, an odd number of launches ends in the scratch copy and costs one device-to-device copy of the
// iterate; with a destination the chain input -> (scratch | dst) ... -> dst needs no copy at all.
template <class Mdl> int run_chain(const SweepCall<Mdl> &c, const SorPlan &plan, float *(&buf)[3][Mdl::NIT])
{
    using PL = RbpLayout<Mdl, PS>;
    SweepPlanes<Mdl> P = c.P;
    hipStream_t s = c.s;
    SweepTimer timer(s, PDEIP_TIMER_MARKERS ? 0 : plan.nlaunch); // the events ride on the first and the last launch: no packet of their own
    int done = 0; // sweeps
    DeviceState *d = cur_dev();
    RC(for_each_launch(plan, [&](const SorLaunch &l) {
        bind_buffers<Mdl>(P, buf, l);
        hipEvent_t const e0 = timer.start_for(l.index), e1 = timer.stop_for(l.index);
        const int mirror = l.kind == K_RBP ? resolve_mirror(plan.mirror_mode, d->rbp_next_mirror) : 0;
        if (l.kind == K_RBP) {
            RC(ensure_lds(reinterpret_cast<const void *>(rbp_kernel<Mdl>(l.first)), PL::LDS_BYTES));
            // the derived planes leave the kernel only if a later launch of this call reads them
            const bool keep = l.first && done + PS < c.iter;
            launch_timed(rbp_kernel<Mdl>(l.first), dim3((unsigned)l.gridx, (unsigned)c.nframes), dim3(PL::THREADS), PL::LDS_BYTES, s, e0, e1, P, keep ? c.aux0 : nullptr,
                         keep ? c.aux1 : nullptr, c.nrows, c.ncols, l.tj, l.tiles, l.units, c.omega, c.col0, c.n, mirror);
        } else { // the first launch also builds the divisor planes
            launch_timed(rb_kernel<Mdl>(plan.vec, l.first, l.sweeps == 2), dim3((unsigned)l.gridx, (unsigned)c.nframes), dim3(64 * RB_WAVES_PER_BLOCK), 0, s, e0, e1, P,
                         l.first ? c.aux0 : nullptr, l.first ? c.aux1 : nullptr, c.nrows, c.ncols, l.tj, l.tiles, l.units, c.omega, c.col0, c.n);
        }
        if (l.first) {
            P.cf[Mdl::D0] = c.aux0;
            P.cf[Mdl::D1] = c.aux1;
        }
        done += l.sweeps;
        tls.last_launches++;
        tls.last_directions.push_back(mirror);
        return PDEIP_OK;
    }));
    timer.stop(plan.nlaunch);
    if (plan.copy_back)
        for (int f = 0; f < Mdl::NIT; f++) RC(copy_d2d(s, buf[BUF_CALLER][f], buf[BUF_SCRATCH][f], c.n * c.nframes));
    HIPCHK(hipGetLastError());
    return PDEIP_OK;
}

// Runs `iter` sweeps of model Mdl on the iterate buffers P.it_out (in place from the caller's point of view): plan, fetch the
// workspace, run the plan's family.
//
// `dst` (optional): NIT buffers that receive the result while the caller's iterate in P.it_out is only READ -- what a
// gateway does anyway (copy in, solve on the output: Oflow_sor_elin4_2d.c:341-346).
template <class Mdl>
int run_sweeps(hipStream_t s, SweepPlanes<Mdl> P, int nrows, int ncols, int nframes, int iter,
               float omega, int mode, int col0, float *const *dst = nullptr)
{
    constexpr int NIT = Mdl::NIT;
    const size_t n = (size_t)nrows * ncols;
    tls.last_launches = 0;
    tls.last_directions.clear();
    bool same = dst != nullptr, aligned = true; // dst == it_out: in place
    for (int f = 0; f < NIT; f++) {
        same = same && dst[f] == P.it_out[f];
        aligned = aligned && aligned16(P.it_out[f]) && (!dst || aligned16(dst[f]));
    }
    if (same) dst = nullptr;
    for (int f = 0; f < Mdl::NCF; f++) aligned = aligned && aligned16(P.cf[f]);
    for (int f = 0; f < Mdl::NRO; f++) aligned = aligned && aligned16(P.ro[f]);
    const SorShape sh{nrows, ncols, nframes, iter, mode, aligned, dst != nullptr, 0, 0};
    const SorPlan plan = plan_for<Mdl>(sh, SorDevice{});
    if (plan.copy_in)
        for (int f = 0; f < NIT; f++) RC(copy_d2d(s, dst[f], P.it_out[f], n * nframes));
    if (plan.family == SOR_NONE) return PDEIP_OK;
    // workspace: the derived planes, and for the chain a scratch copy of the iterate (16-byte aligned like every allocation; a
    // frame of the vector kernels is a multiple of four floats, so every plane in them is too)
    SweepCall<Mdl> c{s, P, nrows, ncols, nframes, iter, omega, col0, n, nullptr, nullptr, dst};
    RC(ws_get(WS_AUX0, n * nframes * sizeof(float), &c.aux0));
    RC(ws_get(WS_AUX1, n * nframes * sizeof(float), &c.aux1));
    if (plan.family == SOR_EXACT) return run_exact(c, plan);
    float *scratch = nullptr;
    if (plan.family != SOR_SMALL) RC(ws_get(WS_PING, (size_t)NIT * n * nframes * sizeof(float), &scratch));
    float *buf[3][NIT];
    for (int f = 0; f < NIT; f++) {
        buf[BUF_CALLER][f] = P.it_out[f];
        buf[BUF_SCRATCH][f] = scratch ? scratch + (size_t)f * n * nframes : nullptr;
        buf[BUF_DST][f] = dst ? dst[f] : nullptr;
    }
    return plan.family == SOR_SMALL ? run_small(c, plan, buf) : run_chain(c, plan, buf);
}

} // namespace

extern "C" int pdeip_debug_plan_sor(int model, int nrows, int ncols, int nframes, int iter, int mode, int aligned16, int has_dst, int num_cus,
                                    int rb2_slots, int rbp_slots, int *info, int *records, int capacity)
{
    const char *who = "pdeip_debug_plan_sor";
    RC(check_dims(who, nrows, ncols, nframes));
    RC(check_mode(who, mode));
    if (info == nullptr || (records == nullptr && capacity > 0)) return set_err(PDEIP_ERR_ARG, "%s: null pointer", who);
    const SorShape sh{nrows, ncols, nframes, iter, mode, aligned16 != 0, has_dst != 0, 0, 0};
    const SorDevice dev{num_cus, rb2_slots, rbp_slots};
    SorPlan p;
    switch (model) {
    case PDEIP_PLAN_ELIN4: p = plan_for<ModelElin4>(sh, dev); break;
    case PDEIP_PLAN_LLIN4: p = plan_for<ModelLlin4>(sh, dev); break;
    case PDEIP_PLAN_DISP4: p = plan_for<ModelDisp4>(sh, dev); break;
    case PDEIP_PLAN_PDE4: p = plan_for<ModelPde4>(sh, dev); break;
    case PDEIP_PLAN_PDE8: p = plan_sor_pde8(sh, dev); break;
    case PDEIP_PLAN_DISPSYM4: p = plan_for<ModelDispSym4>(sh, dev); break;
    default: return set_err(PDEIP_ERR_ARG, "%s: unknown model %d", who, model);
    }
    const int head[PDEIP_PLAN_INFO] = {p.family, p.form, p.copy_back, p.copy_in, p.persist_setup, p.A, p.B, p.NC, p.W, p.last_m, 0};
    memcpy(info, head, sizeof head);
    // pdeip_disp_sor_llin_sym4_dev relaxes its two fields one after the other: the plan, twice
    for (int run = 0; run < (model == PDEIP_PLAN_DISPSYM4 ? 2 : 1); run++)
        (void)for_each_launch(p, [&](const SorLaunch &l) {
            const int rec[PDEIP_PLAN_RECORD] = {l.kind, l.sweeps, l.first, l.tj, l.tiles, l.units, l.gridx, l.src, l.dst};
            if (info[10] < capacity) memcpy(records + (size_t)PDEIP_PLAN_RECORD * info[10], rec, sizeof rec);
            info[10]++;
            return PDEIP_OK;
        });
    return PDEIP_OK;
}

extern "C" int pdeip_debug_persist_order(int B, int T, int affine, int *table)
{
    if (B < 1 || T < 1 || table == nullptr) return set_err(PDEIP_ERR_ARG, "pdeip_debug_persist_order: bad arguments");
    RC(use_device());
    int *dev = nullptr;
    const size_t n = PERSIST_TABLE_HDR + (size_t)B * T;
    HIPCHK(hipMalloc(&dev, n * sizeof(int)));
    hipLaunchKernelGGL(k_persist_order, dim3((unsigned)((B * T + 255) / 256)), dim3(256), 0, nullptr, dev, B, T, affine ? 1 : 0);
    const hipError_t e = hipMemcpy(table, dev, n * sizeof(int), hipMemcpyDeviceToHost);
    (void)hipFree(dev);
    if (e != hipSuccess) return set_err(PDEIP_ERR_DEVICE, "pdeip_debug_persist_order: %s", hipGetErrorString(e));
    return PDEIP_OK;
}

namespace {
__global__ void k_rcp_check(unsigned long long *counts)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    unsigned long long n = 0, bad = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < (1ull << 32); i += stride) {
        const unsigned bits = (unsigned)i;
        const float d = __uint_as_float(bits);
        bool in_range = true;
        RcpRange{in_range}(d);
        if (in_range != (((bits >> 23) & 0xff) >= 1 && ((bits >> 23) & 0xff) <= 252)) bad++; // the range test is the exponent test
        if (!in_range) continue;
        n++;
        if (__float_as_uint(RcpFast()(d)) != __float_as_uint(RcpIeee()(d))) bad++;
    }
    atomicAdd(counts + 0, n);
    atomicAdd(counts + 1, bad);
}
} // namespace

extern "C" int pdeip_debug_rcp_check(unsigned long long *counts)
{
    if (counts == nullptr) return set_err(PDEIP_ERR_ARG, "pdeip_debug_rcp_check: null pointer");
    RC(use_device());
    unsigned long long *dev = nullptr;
    HIPCHK(hipMalloc(&dev, 2 * sizeof(unsigned long long)));
    hipError_t e = hipMemset(dev, 0, 2 * sizeof(unsigned long long));
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_rcp_check, dim3(4096), dim3(256), 0, nullptr, dev);
        e = hipMemcpy(counts, dev, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    }
    (void)hipFree(dev);
    if (e != hipSuccess) return set_err(PDEIP_ERR_DEVICE, "pdeip_debug_rcp_check: %s", hipGetErrorString(e));
    return PDEIP_OK;
}

#ifdef PDEIP_RBP_STAMPS
extern "C" int pdeip_debug_read_rbp_stamps(unsigned long long *out)
{
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rbp_stamps), 256 * sizeof(unsigned long long)));
    return PDEIP_OK;
}
#endif
#ifdef PDEIP_P8_STAMPS
extern "C" int pdeip_debug_read_walk_stamps(unsigned long long *out)
{
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_p8_stamps), 4096 * sizeof(unsigned long long)));
    return PDEIP_OK;
}
#endif
#ifdef PDEIP_EXACT_STAMPS
extern "C" int pdeip_debug_read_stamps(unsigned long long *out)
{
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_exact_stamps), 64 * sizeof(unsigned long long)));
    return PDEIP_OK;
}
#endif

// ------------------------------------------------------------------------------------------------
// device-pointer entry points
// ------------------------------------------------------------------------------------------------
// Every 5-point solver has two device entry points: `_dev` relaxes the iterate in place, `_dev_to` reads the iterate and writes
// the relaxed one to separate planes (iter <= 0: a copy) -- the gateway's own shape (copy in, solve on the output) and, for the
// red-black launches, the one that needs no device-to-device copy of the iterate (run_sweeps).
extern "C" int pdeip_oflow_sor_elin4_dev_to(void *stream, const float *U, const float *V, float *U_out, float *V_out, const float *M,
                                            const float *Cu, const float *Cv, const float *Du, const float *Dv, const float *wW,
                                            const float *wN, const float *wE, const float *wS, int nrows, int ncols, int iter,
                                            float omega, int mode, int col0)
{
    const char *who = "pdeip_oflow_sor_elin4_dev";
    RC(check_dims(who, nrows, ncols, 1));
    RC(check_mode(who, mode));
    hipStream_t s = static_cast<hipStream_t>(stream);
    SweepPlanes<ModelElin4> P{};
    P.it_out[0] = const_cast<float *>(U);
    P.it_out[1] = const_cast<float *>(V);
    const float *cf[9] = {M, Cu, Cv, Du, Dv, wW, wN, wE, wS}; // Du,Dv: raw planes in the divisor slots
    for (int f = 0; f < 9; f++) P.cf[f] = cf[f];
    float *const dst[2] = {U_out, V_out};
    RC(run_sweeps<ModelElin4>(s, P, nrows, ncols, 1, iter, omega, mode, col0, dst));
    return PDEIP_OK;
}
extern "C" int pdeip_oflow_sor_elin4_dev(void *stream, float *U, float *V, const float *M, const float *Cu,
                                         const float *Cv, const float *Du, const float *Dv, const float *wW,
                                         const float *wN, const float *wE, const float *wS, int nrows,
                                         int ncols, int iter, float omega, int mode, int col0)
{
    return pdeip_oflow_sor_elin4_dev_to(stream, U, V, U, V, M, Cu, Cv, Du, Dv, wW, wN, wE, wS, nrows, ncols, iter, omega, mode, col0);
}

extern "C" int pdeip_oflow_sor_llin4_dev_to(void *stream, const float *U, const float *V, const float *dU, const float *dV,
                                            float *dU_out, float *dV_out, const float *M, const float *Cu, const float *Cv,
                                            const float *Du, const float *Dv, const float *wW, const float *wN, const float *wE,
                                            const float *wS, int nrows, int ncols, int iter, float omega, int mode, int col0)
{
    const char *who = "pdeip_oflow_sor_llin4_dev";
    RC(check_dims(who, nrows, ncols, 1));
    RC(check_mode(who, mode));
    hipStream_t s = static_cast<hipStream_t>(stream);
    SweepPlanes<ModelLlin4> P{};
    P.it_out[0] = const_cast<float *>(dU);
    P.it_out[1] = const_cast<float *>(dV);
    P.ro[0] = U;
    P.ro[1] = V;
    const float *cf[9] = {M, Cu, Cv, Du, Dv, wW, wN, wE, wS}; // Du,Dv: raw planes in the divisor slots
    for (int f = 0; f < 9; f++) P.cf[f] = cf[f];
    float *const dst[2] = {dU_out, dV_out};
    RC(run_sweeps<ModelLlin4>(s, P, nrows, ncols, 1, iter, omega, mode, col0, dst));
    return PDEIP_OK;
}
extern "C" int pdeip_oflow_sor_llin4_dev(void *stream, const float *U, const float *V, float *dU, float *dV,
                                         const float *M, const float *Cu, const float *Cv, const float *Du,
                                         const float *Dv, const float *wW, const float *wN, const float *wE,
                                         const float *wS, int nrows, int ncols, int iter, float omega,
                                         int mode, int col0)
{
    return pdeip_oflow_sor_llin4_dev_to(stream, U, V, dU, dV, dU, dV, M, Cu, Cv, Du, Dv, wW, wN, wE, wS, nrows, ncols, iter, omega, mode, col0);
}

extern "C" int pdeip_disp_sor_llin4_dev_to(void *stream, const float *U, const float *dU, float *dU_out, const float *Cu,
                                           const float *Du, const float *wW, const float *wN, const float *wE, const float *wS,
                                           int nrows, int ncols, int iter, float omega, int mode, int col0)
{
    const char *who = "pdeip_disp_sor_llin4_dev";
    RC(check_dims(who, nrows, ncols, 1));
    RC(check_mode(who, mode));
    hipStream_t s = static_cast<hipStream_t>(stream);
    SweepPlanes<ModelDisp4> P{};
    P.it_out[0] = const_cast<float *>(dU);
    P.ro[0] = U;
    const float *cf[6] = {Cu, Du, wW, wN, wE, wS}; // Cu,Du: raw planes in the dividend/divisor slots
    for (int f = 0; f < 6; f++) P.cf[f] = cf[f];
    float *const dst[1] = {dU_out};
    RC(run_sweeps<ModelDisp4>(s, P, nrows, ncols, 1, iter, omega, mode, col0, dst));
    return PDEIP_OK;
}
extern "C" int pdeip_disp_sor_llin4_dev(void *stream, const float *U, float *dU, const float *Cu,
                                        const float *Du, const float *wW, const float *wN, const float *wE,
                                        const float *wS, int nrows, int ncols, int iter, float omega,
                                        int mode, int col0)
{
    return pdeip_disp_sor_llin4_dev_to(stream, U, dU, dU, Cu, Du, wW, wN, wE, wS, nrows, ncols, iter, omega, mode, col0);
}

// Disp_sor_llin_sym4_2d: two disparity fields that do not read each other (disparitySolvers.c:301-548).
// solver 1: ModelDispSym4 on each; solver 2: the line solvers are the plain disparity ones (:503-540).
extern "C" int pdeip_disp_sor_llin_sym4_dev(void *stream, const float *U0, float *dU0, const float *Cu0, const float *Du0,
                                            const float *wW0, const float *wN0, const float *wE0, const float *wS0,
                                            const float *U1, float *dU1, const float *Cu1, const float *Du1,
                                            const float *wW1, const float *wN1, const float *wE1, const float *wS1,
                                            int nrows, int ncols, int iter, float omega, int solver, int mode, int col0)
{
    const char *who = "pdeip_disp_sor_llin_sym4_dev";
    RC(check_dims(who, nrows, ncols, 1));
    RC(check_mode(who, mode));
    RC(check_solver(who, solver));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (iter <= 0) return PDEIP_OK;
    const float *U[2] = {U0, U1}, *cf[2][6] = {{Cu0, Du0, wW0, wN0, wE0, wS0}, {Cu1, Du1, wW1, wN1, wE1, wS1}};
    float *dU[2] = {dU0, dU1};
    int launches = 0;
    std::vector<int> directions; // of both fields' launches, in order
    for (int k = 0; k < 2; k++) {
        if (solver == PDEIP_SOLVER_ALR) {
            RC(pdeip_disp_alr_llin4_dev(stream, U[k], dU[k], cf[k][0], cf[k][1], cf[k][2], cf[k][3], cf[k][4], cf[k][5], nrows, ncols, iter, omega, mode));
        } else {
            SweepPlanes<ModelDispSym4> P{};
            P.it_out[0] = dU[k];
            P.ro[0] = U[k];
            for (int f = 0; f < 6; f++) P.cf[f] = cf[k][f];
            RC(run_sweeps<ModelDispSym4>(s, P, nrows, ncols, 1, iter, omega, mode, col0));
            directions.insert(directions.end(), tls.last_directions.begin(), tls.last_directions.end());
        }
        launches += tls.last_launches;
    }
    tls.last_launches = launches;
    tls.last_directions = directions;
    return PDEIP_OK;
}

extern "C" int pdeip_pde_sor4_dev_to(void *stream, const float *X, float *X_out, const float *TRACE, const float *B, const float *wW,
                                     const float *wN, const float *wE, const float *wS, int nrows, int ncols, int nframes, int iter,
                                     float omega, int mode, int col0)
{
    const char *who = "pdeip_pde_sor4_dev";
    RC(check_dims(who, nrows, ncols, nframes));
    RC(check_mode(who, mode));
    hipStream_t s = static_cast<hipStream_t>(stream);
    SweepPlanes<ModelPde4> P{};
    P.it_out[0] = const_cast<float *>(X);
    const float *cf[6] = {B, TRACE, wW, wN, wE, wS}; // B,TRACE: raw planes in the derived slots
    for (int f = 0; f < 6; f++) P.cf[f] = cf[f];
    float *const dst[1] = {X_out};
    RC(run_sweeps<ModelPde4>(s, P, nrows, ncols, nframes, iter, omega, mode, col0, dst));
    return PDEIP_OK;
}
extern "C" int pdeip_pde_sor4_dev(void *stream, float *X, const float *TRACE, const float *B, const float *wW,
                                  const float *wN, const float *wE, const float *wS, int nrows, int ncols,
                                  int nframes, int iter, float omega, int mode, int col0)
{
    return pdeip_pde_sor4_dev_to(stream, X, X, TRACE, B, wW, wN, wE, wS, nrows, ncols, nframes, iter, omega, mode, col0);
}

