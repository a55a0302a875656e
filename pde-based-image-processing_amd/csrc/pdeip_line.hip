// pdeip_line.hip -- libpdeip.so: alternating line relaxation (solver = 2): launch logic and the *_dev entry points.
//
// Build (build.py): hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -c, one object per translation unit.
// -ffp-contract=off is part of the parity contract: the reference is plain C built without FMA.
#include "pdeip_ctx.hpp"

#include "pdeip_alr.hpp"

using namespace pdeip;

// ------------------------------------------------------------------------------------------------
// alternating line relaxation (solver 2): kernels in pdeip_alr.hpp, the decision in pdeip_alr_plan.hpp
// ------------------------------------------------------------------------------------------------

// The fields a model's solver couples: the chains of one launch (elin4, llin4 and llin8 solve U and V together).
template <class Mdl>
constexpr int ALR_MODEL_CHAINS = (std::is_same<Mdl, AlrElin4>::value || std::is_same<Mdl, AlrLlin4>::value || std::is_same<Mdl, AlrLlin8>::value) ? 2 : 1;

template <class Mdl> constexpr AlrTraits alr_traits() { return AlrTraits{ALR_MODEL_CHAINS<Mdl>, Mdl::INTERIOR_LINES}; }

// Every launch of this file: the LDS opt-in where the plan asks for it, the launch, the count.  The caller asks for the error
// state once its launches are out (alr_launched).
template <class... KArgs, class... Args>
static int alr_launch(void (*kernel)(KArgs...), dim3 grid, int threads, size_t lds, bool opt_in, hipStream_t s, const Args &...args)
{
    if (opt_in) RC(ensure_lds(reinterpret_cast<const void *>(kernel), lds));
    hipLaunchKernelGGL(kernel, grid, dim3(threads), lds, s, static_cast<KArgs>(args)...);
    tls.last_launches++;
    return PDEIP_OK;
}
static int alr_launched()
{
    HIPCHK(hipGetLastError());
    return PDEIP_OK;
}
// `vertical` and G as template arguments: fn(std::true_type{}) / fn(std::integral_constant<int, G>{})
template <class F> static int by_direction(bool vertical, F &&fn) { return vertical ? fn(std::true_type{}) : fn(std::false_type{}); }
template <class F> static int by_groups(int G, F &&fn)
{
    return G == 1 ? fn(std::integral_constant<int, 1>{}) : (G == 2 ? fn(std::integral_constant<int, 2>{}) : fn(std::integral_constant<int, 3>{}));
}

// Workspace of one call (WS_ALR): per (chain, direction) the cp and divisor planes (k_alr_zebra3<ZB_FACTOR>), the part of the
// Thomas recurrence that depends on the coefficient planes only.
struct AlrFactors {
    float *cp[2][2], *dv[2][2]; // [chain][vertical ? 0 : 1]
};
static void alr_carve_factors(float *base, size_t plane, int nch, float *(&cp)[2][2], float *(&dv)[2][2])
{
    for (int c = 0; c < nch; c++)
        for (int d = 0; d < 2; d++) {
            cp[c][d] = base + plane * (size_t)((c * 2 + d) * 2);
            dv[c][d] = cp[c][d] + plane;
        }
}

// The chains of one launch: the fields order[0..NCH) with their factor planes of direction d.
template <class Mdl, int NCH>
static AlrChains<Mdl, NCH> alr_chains(const typename Mdl::Ctx *q, float *const *x, const AlrFactors &f, const int *order, int d)
{
    AlrChains<Mdl, NCH> ch;
    for (int c = 0; c < NCH; c++) ch.c[c] = AlrChain<Mdl>{q[order[c]], x[order[c]], f.cp[order[c]][d], f.dv[order[c]][d]};
    return ch;
}

// The row passes run on transposed copies of every plane (pdeip_alr.hpp).  A model's Ctx is a plain
// struct of plane pointers; each distinct plane gets one transposed twin in the WS_ALR_T workspace.  The
// coefficient planes are transposed once per call, the iterate planes around every row pass.
struct AlrTwin {
    static constexpr int MAXP = 40;
    const float *orig[MAXP];
    float *twin[MAXP];
    int count = 0, ncoef = 0; // ncoef: those that are no iterate
    float *find(const float *p) const
    {
        for (int k = 0; k < count; k++)
            if (orig[k] == p) return twin[k];
        return nullptr;
    }
};

// Registers every distinct plane of the call.  No HIP call, and membership is asked of orig[] alone: the twins are carved once
// the plan has said how much workspace the call takes (alr_make_twins).
template <class Ctx> static int alr_register(AlrTwin *tw, const Ctx *q, int nch, float *const *x)
{
    static_assert(sizeof(Ctx) % sizeof(float *) == 0, "a line-relaxation context is a struct of plane pointers");
    constexpr int NP = (int)(sizeof(Ctx) / sizeof(float *));
    for (int c = 0; c < nch; c++) {
        const float *ptrs[NP];
        memcpy(ptrs, &q[c], sizeof(Ctx));
        for (int k = 0; k < NP; k++) {
            bool seen = ptrs[k] == nullptr;
            for (int j = 0; j < tw->count && !seen; j++) seen = tw->orig[j] == ptrs[k];
            if (seen) continue;
            if (tw->count == AlrTwin::MAXP) return set_err(PDEIP_ERR_ARG, "line relaxation: too many planes");
            tw->orig[tw->count++] = ptrs[k];
            bool iterate = false;
            for (int j = 0; j < nch; j++) iterate = iterate || ptrs[k] == x[j];
            if (!iterate) tw->ncoef++;
        }
    }
    return PDEIP_OK;
}

// The twins in the workspace at `base`, the transposed contexts qt / iterates xt, and the coefficient planes (in -> out, ncoef of
// them) that are transposed once per call.
template <class Ctx>
static void alr_make_twins(AlrTwin *tw, float *base, size_t plane, const Ctx *q, Ctx *qt, int nch, float *const *x, float **xt, const float **ins, float **outs)
{
    constexpr int NP = (int)(sizeof(Ctx) / sizeof(float *));
    int nco = 0;
    for (int k = 0; k < tw->count; k++) {
        tw->twin[k] = base + plane * k;
        bool iterate = false;
        for (int c = 0; c < nch; c++) iterate = iterate || tw->orig[k] == x[c];
        if (!iterate) {
            outs[nco] = tw->twin[k];
            ins[nco++] = tw->orig[k];
        }
    }
    for (int c = 0; c < nch; c++) {
        const float *ptrs[NP], *tp[NP];
        memcpy(ptrs, &q[c], sizeof(Ctx));
        for (int k = 0; k < NP; k++) tp[k] = ptrs[k] ? tw->find(ptrs[k]) : nullptr;
        memcpy(&qt[c], tp, sizeof(Ctx));
        xt[c] = tw->find(x[c]);
    }
}

// out[k] = in[k] transposed, up to ALR_TB_MAX planes per launch
static int alr_transpose_many(hipStream_t s, float *const *out, const float *const *in, int count, int na, int nb, int nframes)
{
    for (int k0 = 0; k0 < count; k0 += ALR_TB_MAX) {
        AlrTransposeBatch B{};
        const int m = count - k0 < ALR_TB_MAX ? count - k0 : ALR_TB_MAX;
        for (int k = 0; k < m; k++) {
            B.out[k] = out[k0 + k];
            B.in[k] = in[k0 + k];
        }
        RC(alr_launch(k_alr_transpose_batch, dim3((unsigned)((na + 31) / 32), (unsigned)((nb + 31) / 32), (unsigned)(m * nframes)), 256, 0, false, s, B, na,
                      nb, nframes));
    }
    return alr_launched();
}

// What the launches of one call share.  q / x: contexts and iterates as the caller has them, qt / xt: their transposed twins.
template <class Mdl> struct AlrCall {
    hipStream_t s;
    const typename Mdl::Ctx *q, *qt;
    float *const *x, *const *xt;
    AlrFactors f;
    float *dp, *gline; // WS_AUX1 (zebra), WS_LEX (the global line buffer)
    int nch, nrows, ncols, nframes;
    float omega;
};

// cp and divisor planes of every (field, direction), once per call.  Column planes from q, row planes from the transposed qt.
template <class Mdl> static int alr_factor(const AlrCall<Mdl> &c, const AlrPlan &plan)
{
    const size_t fs = (size_t)c.nrows * c.ncols;
    for (int ch = 0; ch < (plan.factor_pair ? 1 : c.nch); ch++) // both fields of a coupled solver in one launch per direction
        for (int d = 0; d < 2; d++)
            RC(by_direction(d == 0, [&](auto V) {
                constexpr bool VERT = decltype(V)::value;
                const typename Mdl::Ctx *q = VERT ? c.q : c.qt;
                const AlrPass &p = plan.pass[d];
                if (plan.factor_pair)
                    return alr_launch(k_alr_factor_pair<Mdl, VERT>, dim3((unsigned)p.factor_gridx, (unsigned)c.nframes, 2), ZB_THREADS, Z3_LDS_BYTES, false,
                                      c.s, q[0], q[1], c.f.cp[0][d], c.f.dv[0][d], c.f.cp[1][d], c.f.dv[1][d], c.nrows, c.ncols, fs, p.lo, p.hi);
                return alr_launch(k_alr_zebra3<Mdl, VERT, ZB_FACTOR>, dim3((unsigned)p.factor_gridx, (unsigned)c.nframes), ZB_THREADS, Z3_LDS_BYTES, false, c.s,
                                  q[ch], nullptr, c.f.cp[ch][d], c.f.dv[ch][d], nullptr, c.nrows, c.ncols, fs, p.lo, p.hi, 1, 0.0f);
            }));
    return alr_launched();
}

// One direction of one iteration, as its pass record says.
template <class Mdl> static int alr_pass(const AlrCall<Mdl> &c, const AlrPass &p, bool vertical)
{
    RC(by_direction(vertical, [&](auto V) {
        constexpr bool VERT = decltype(V)::value;
        constexpr int d = VERT ? 0 : 1;
        const typename Mdl::Ctx *q = VERT ? c.q : c.qt;
        float *const *x = VERT ? c.x : c.xt;
        const AlrFactors &f = c.f;
        const int nrows = c.nrows, ncols = c.ncols, a = p.order[0], b = p.order[1];
        const size_t fs = (size_t)nrows * ncols;
        const dim3 frames((unsigned)p.gridx);
        switch (p.kind) {
        case AK_ZEBRA3: // one field after the other: even lines, then odd lines
            for (int i = 0; i < c.nch; i++)
                for (int k = 0; k < p.ncolours; k++)
                    RC(alr_launch(k_alr_zebra3<Mdl, VERT, ZB_APPLY>, dim3((unsigned)p.colour[k].gridx, (unsigned)c.nframes), ZB_THREADS, p.lds, p.opt_in, c.s,
                                  q[p.order[i]], x[p.order[i]], f.cp[p.order[i]][d], f.dv[p.order[i]][d], c.dp, nrows, ncols, fs, p.colour[k].first,
                                  p.colour[k].last, 2, c.omega));
            return PDEIP_OK;
        case AK_ZEBRA3_PAIR: // field a first, then field b, as the per-field passes would run them
            for (int k = 0; k < p.ncolours; k++)
                RC(alr_launch(k_alr_zebra3_pair<Mdl, VERT, ZB_APPLY>, dim3((unsigned)p.colour[k].gridx, (unsigned)c.nframes), ZB_THREADS, p.lds, p.opt_in, c.s,
                              q[a], x[a], f.cp[a][d], f.dv[a][d], q[b], x[b], f.cp[b][d], f.dv[b][d], c.dp, nrows, ncols, fs, p.colour[k].first,
                              p.colour[k].last, 2, c.omega));
            return PDEIP_OK;
        case AK_LEX: // reference line order; chain 1 trails chain 0 by a line
            if (p.chains == 2)
                return alr_launch(k_alr_lex<Mdl, 2, VERT>, frames, ALR_LEX_THREADS, p.lds, p.opt_in, c.s, alr_chains<Mdl, 2>(q, x, f, p.order, d), nrows, ncols,
                                  fs, p.lo, p.hi, c.omega, nullptr);
            for (int i = 0; i < c.nch; i++)
                RC(alr_launch(k_alr_lex<Mdl, 1, VERT>, frames, ALR_LEX_THREADS, p.lds, p.opt_in, c.s, alr_chains<Mdl, 1>(q, x, f, p.order + i, d), nrows, ncols,
                              fs, p.lo, p.hi, c.omega, nullptr));
            return PDEIP_OK;
        case AK_LEX_GLOBAL:
            for (int i = 0; i < c.nch; i++)
                RC(alr_launch(k_alr_lex<Mdl, 1, VERT, true>, frames, ALR_LEX_THREADS, 0, false, c.s, alr_chains<Mdl, 1>(q, x, f, p.order + i, d), nrows, ncols, fs,
                              p.lo, p.hi, c.omega, reinterpret_cast<float4 *>(c.gline)));
            return PDEIP_OK;
        default: // AK_SCAN: all chains in one launch, G groups of four elements per lane
            return by_groups(p.G, [&](auto G) {
                constexpr int NCH = ALR_MODEL_CHAINS<Mdl>;
                return alr_launch(k_alr_scan<Mdl, NCH, VERT, decltype(G)::value>, frames, ALR_SCAN_THREADS, 0, false, c.s, alr_chains<Mdl, NCH>(q, x, f, p.order, d),
                                  nrows, ncols, fs, p.lo, p.hi, c.omega);
            });
        }
    }));
    return alr_launched();
}

// Every line-relaxation entry point.  q[c] / x[c]: context and iterate plane of field c.  Checks, registers the call's planes,
// plans (pdeip_alr_plan.hpp), fetches the workspace the plan names and runs the plan's launches.
template <class Mdl>
static int run_alr(const char *who, hipStream_t s, const typename Mdl::Ctx *q, float *const *x, int nch, int nrows, int ncols,
                   int nframes, int iter, float omega, int mode)
{
    RC(check_dims(who, nrows, ncols, nframes));
    RC(check_mode(who, mode));
    tls.last_launches = 0;
    if (iter <= 0) return PDEIP_OK;
    AlrTwin tw;
    RC(alr_register(&tw, q, nch, x));
    const AlrPlan plan = plan_alr(alr_traits<Mdl>(), AlrShape{nrows, ncols, nframes, iter, mode, nch, tw.count, tw.ncoef}, alr_knobs(env_int));
    const size_t fs = (size_t)nrows * ncols;
    typename Mdl::Ctx qt[2];
    float *xt[2] = {nullptr, nullptr}, *fbase, *tbase, *tout[AlrTwin::MAXP];
    const float *tin[AlrTwin::MAXP];
    AlrCall<Mdl> c{s, q, qt, x, xt, AlrFactors{}, nullptr, nullptr, nch, nrows, ncols, nframes, omega};
    RC(ws_get(WS_ALR, plan.ws_alr * sizeof(float), &fbase));
    RC(ws_get(WS_ALR_T, plan.ws_alr_t * sizeof(float), &tbase));
    if (plan.ws_aux1) RC(ws_get(WS_AUX1, plan.ws_aux1 * sizeof(float), &c.dp));
    if (plan.ws_lex) RC(ws_get(WS_LEX, plan.ws_lex * sizeof(float), &c.gline));
    alr_carve_factors(fbase, fs * nframes, nch, c.f.cp, c.f.dv);
    alr_make_twins(&tw, tbase, fs * nframes, q, qt, nch, x, xt, tin, tout);
    if (plan.family == ALR_SMALL) { // the kernel transposes the coefficient planes itself
        AlrSmallArgs<Mdl> A{};
        for (int k = 0; k < nch; k++) {
            A.q[k] = q[k];
            A.qt[k] = qt[k];
            A.x[k] = x[k];
            A.xt[k] = xt[k];
        }
        memcpy(A.cp, c.f.cp, sizeof A.cp);
        memcpy(A.dv, c.f.dv, sizeof A.dv);
        for (int k = 0; k < tw.ncoef; k++) {
            A.tin[k] = tin[k];
            A.tout[k] = tout[k];
        }
        A.ntr = tw.ncoef; A.nch = nch; A.nrows = nrows; A.ncols = ncols; A.iter = iter; A.omega = omega;
        A.fs = fs;
        if (plan.small_opt_in) RC(ensure_lds(reinterpret_cast<const void *>(&k_alr_small<Mdl>), plan.small_lds)); // ahead of the timed bracket
        SweepTimer timer(s);
        RC(alr_launch(k_alr_small<Mdl>, dim3((unsigned)nframes), ALR_SMALL_THREADS, plan.small_lds, false, s, A));
        timer.stop(iter);
        return alr_launched();
    }
    RC(alr_transpose_many(s, tout, tin, tw.ncoef, nrows, ncols, nframes));
    RC(alr_factor(c, plan));
    SweepTimer timer(s);
    for (int it = 0; it < iter; it++) { // columns, the iterate to its twin, rows, and back
        RC(alr_pass(c, plan.pass[0], true));
        RC(alr_transpose_many(s, xt, x, nch, nrows, ncols, nframes));
        RC(alr_pass(c, plan.pass[1], false));
        RC(alr_transpose_many(s, x, xt, nch, ncols, nrows, nframes));
    }
    timer.stop(iter);
    return PDEIP_OK;
}

extern "C" int pdeip_oflow_alr_elin4_dev(void *stream, float *U, float *V, const float *M, const float *Cu,
                                         const float *Cv, const float *Du, const float *Dv, const float *wW,
                                         const float *wN, const float *wE, const float *wS, int nrows, int ncols,
                                         int iter, float omega, int mode)
{
    const AlrElin4::Ctx q[2] = {{U, V, M, Cu, Du, wW, wN, wE, wS}, {V, U, M, Cv, Dv, wW, wN, wE, wS}};
    float *const x[2] = {U, V};
    return run_alr<AlrElin4>("pdeip_oflow_alr_elin4_dev", static_cast<hipStream_t>(stream), q, x, 2, nrows, ncols, 1, iter, omega, mode);
}

extern "C" int pdeip_oflow_alr_llin4_dev(void *stream, const float *U, const float *V, float *dU, float *dV,
                                         const float *M, const float *Cu, const float *Cv, const float *Du,
                                         const float *Dv, const float *wW, const float *wN, const float *wE,
                                         const float *wS, int nrows, int ncols, int iter, float omega, int mode)
{
    const AlrLlin4::Ctx q[2] = {{U, dU, dV, M, Cu, Du, wW, wN, wE, wS}, {V, dV, dU, M, Cv, Dv, wW, wN, wE, wS}};
    float *const x[2] = {dU, dV};
    return run_alr<AlrLlin4>("pdeip_oflow_alr_llin4_dev", static_cast<hipStream_t>(stream), q, x, 2, nrows, ncols, 1, iter, omega, mode);
}

extern "C" int pdeip_oflow_alr_llin8_dev(void *stream, const float *U, const float *V, float *dU, float *dV,
                                         const float *M, const float *Cu, const float *Cv, const float *Du,
                                         const float *Dv, const float *wW, const float *wNW, const float *wN,
                                         const float *wNE, const float *wE, const float *wSE, const float *wS,
                                         const float *wSW, int nrows, int ncols, int iter, float omega, int mode)
{
    const AlrLlin8::Ctx q[2] = {{U, dU, dV, M, Cu, Du, {wN, wS, wE, wW, wNW, wNE, wSW, wSE}},
                                {V, dV, dU, M, Cv, Dv, {wN, wS, wE, wW, wNW, wNE, wSW, wSE}}};
    float *const x[2] = {dU, dV};
    return run_alr<AlrLlin8>("pdeip_oflow_alr_llin8_dev", static_cast<hipStream_t>(stream), q, x, 2, nrows, ncols, 1, iter, omega, mode);
}

extern "C" int pdeip_disp_alr_llin4_dev(void *stream, const float *U, float *dU, const float *Cu, const float *Du,
                                        const float *wW, const float *wN, const float *wE, const float *wS,
                                        int nrows, int ncols, int iter, float omega, int mode)
{
    const AlrDisp4::Ctx q[1] = {{U, dU, nullptr, nullptr, Cu, Du, wW, wN, wE, wS}};
    float *const x[1] = {dU};
    return run_alr<AlrDisp4>("pdeip_disp_alr_llin4_dev", static_cast<hipStream_t>(stream), q, x, 1, nrows, ncols, 1, iter, omega, mode);
}

extern "C" int pdeip_pde_alr4_dev(void *stream, float *X, const float *TRACE, const float *B, const float *wW,
                                  const float *wN, const float *wE, const float *wS, int nrows, int ncols,
                                  int nframes, int iter, float omega, int mode)
{
    const AlrPde4::Ctx q[1] = {{X, TRACE, B, wW, wN, wE, wS}};
    float *const x[1] = {X};
    return run_alr<AlrPde4>("pdeip_pde_alr4_dev", static_cast<hipStream_t>(stream), q, x, 1, nrows, ncols, nframes, iter, omega, mode);
}

// One iteration whatever `iter` says (pdeSolvers.c:362), interior columns then interior rows.
extern "C" int pdeip_pde_alr8_dev(void *stream, float *X, const float *TRACE, const float *B, const float *wW,
                                  const float *wNW, const float *wN, const float *wNE, const float *wE,
                                  const float *wSE, const float *wS, const float *wSW, int nrows, int ncols,
                                  int nframes, int iter, float omega, int mode)
{
    (void)iter;
    const AlrPde8::Ctx q[1] = {{X, TRACE, B, wW, wNW, wN, wNE, wE, wSE, wS, wSW}};
    float *const x[1] = {X};
    return run_alr<AlrPde8>("pdeip_pde_alr8_dev", static_cast<hipStream_t>(stream), q, x, 1, nrows, ncols, nframes, 1, omega, mode);
}


// The plan of the call a gateway would make: its model's traits, its fields and its planes (the pointer arguments of the model's
// *_dev entry point, all distinct), and the 9-point model's one iteration.  No HIP call, and nothing of the library's state changes.
extern "C" int pdeip_debug_plan_alr(int model, int nrows, int ncols, int nframes, int iter, int mode, int *info, int *passes)
{
    const char *who = "pdeip_debug_plan_alr";
    static const struct { AlrTraits traits; int nplanes; } MODELS[] = {
        {alr_traits<AlrElin4>(), 11}, {alr_traits<AlrLlin4>(), 13}, {alr_traits<AlrLlin8>(), 17},
        {alr_traits<AlrDisp4>(), 8},  {alr_traits<AlrPde4>(), 7},   {alr_traits<AlrPde8>(), 11}};
    if (info == nullptr || passes == nullptr) return set_err(PDEIP_ERR_ARG, "%s: null pointer", who);
    if (model < 0 || model > PDEIP_PLAN_ALR_PDE8) return set_err(PDEIP_ERR_ARG, "%s: unknown model %d", who, model);
    const bool pde = model >= PDEIP_PLAN_ALR_PDE4;
    RC(check_dims(who, nrows, ncols, pde ? nframes : 1));
    RC(check_mode(who, mode));
    const AlrTraits &t = MODELS[model].traits;
    const AlrShape sh{nrows, ncols, pde ? nframes : 1, model == PDEIP_PLAN_ALR_PDE8 ? 1 : iter, mode, t.chains, MODELS[model].nplanes,
                      MODELS[model].nplanes - t.chains};
    const AlrPlan p = plan_alr(t, sh, alr_knobs(env_int));
    const auto n = [](size_t v) { return v > 0x7fffffff ? 0x7fffffff : (int)v; };
    const int head[PDEIP_PLAN_ALR_INFO] = {p.family, p.nlaunch, p.coef_transposes, p.factor_launches, p.factor_pair, p.iterate_transposes, n(p.small_lds),
                                           p.small_opt_in, n(p.ws_alr), n(p.ws_alr_t), n(p.ws_aux1), n(p.ws_lex)};
    memcpy(info, head, sizeof head);
    for (int d = 0; d < 2; d++) {
        const AlrPass &q = p.pass[d];
        const int rec[PDEIP_PLAN_ALR_PASS] = {q.kind, q.lo, q.hi, q.n, q.factor_gridx, q.ncolours, q.colour[0].first, q.colour[0].last, q.colour[0].gridx,
                                              q.colour[1].first, q.colour[1].last, q.colour[1].gridx, q.chains, q.launches, q.G, n(q.lds), q.opt_in, q.gridx,
                                              q.order[0], q.order[1]};
        memcpy(passes + (size_t)PDEIP_PLAN_ALR_PASS * d, rec, sizeof rec);
    }
    return PDEIP_OK;
}
