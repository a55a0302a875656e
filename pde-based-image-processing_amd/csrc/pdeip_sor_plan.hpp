// pdeip_sor_plan.hpp -- point SOR: what a call launches, decided before the first launch.
//
// plan_sor() turns a call's shape, the knobs and three facts about the device into a SorPlan: the kernel family, the exact-order
// form, and the launches in order with their strip widths, grids and buffers.  It makes no HIP call and reads nothing but its
// arguments and the knobs (the PDEIP_* environment, Context::rb_tj); a device fact it needs and was not given it asks of the
// caller's `ask`, so pdeip_debug_plan_sor() can answer on a machine without a GPU (tests/test_sor_plan.py compares it with
// tests/seam_model.py).  run_sweeps (pdeip_sor5.hip) and pdeip_pde_sor8_dev (pdeip_sor9.hip) plan, fetch workspace and loop
// over the plan with for_each_launch().
#pragma once
#include "pdeip_ctx.hpp"
#include "pdeip_sor_exact.hpp"
#include "pdeip_sor_rb.hpp"
#include "pdeip_sor_small.hpp"

namespace pdeip {

enum { SOR_NONE = 0, SOR_EXACT, SOR_SMALL, SOR_RB, SOR_RBP, SOR_PDE8 }; // family (SOR_RBP: the pipeline, its 2 / 1 tail runs k_sor_rb)
enum { FORM_NONE = 0, FORM_PERSIST, FORM_WALK, FORM_FRONT };             // exact order: one launch, the walker, one launch per front
enum { K_RBP = 1, K_RB2, K_RB1, K_SMALL, K_P8C2, K_P8C1, K_PACK, K_PERSIST, K_WALK, K_DERIVE, K_FRONT, K_BORDERS }; // kernel of a launch
enum { BUF_CALLER = 0, BUF_SCRATCH, BUF_DST };
constexpr int RBP_SWEEPS = 4; // sweeps per launch of the pipeline (k_sor_rbp)
constexpr int MIRROR_ALTERNATE = 3; // PDEIP_RBP_SERPENTINE: every other k_sor_rbp launch on a device marches every strip backwards

// What the planner knows of a model (sor_traits<Mdl>() in pdeip_sor5.hip, PDE8_TRAITS in pdeip_sor9.hip).
struct SorTraits {
    int nit, ncf;
    bool pde8;                                // nine-point: own kernels, in place only, no small path, no pipeline
    int ex_skew;                              // exact order: rows per lane; a front is m = a + (skew + 1) b + (skew + 2) t
    int rb2_own;                              // rows a unit of the two-sweep march owns
    bool rbp_fits;                            // RbpLayout: the rings fit in LDS
    int rbp_nw, rbp_own, rbp_tail;            // waves per sweep, rows a unit owns, nsteps(TJ) - TJ
    SmallPlan (*small)(int, int, int, int);   // SmallLayout::plan
    int (*walk_width)(int, int, int, int);    // the walker's strip width (pdeip_walk_host.hpp)
};
struct SorShape {
    int nrows, ncols, nframes, iter, mode;
    bool aligned16, has_dst;                  // every plane of the caller's 16-byte aligned; a destination that is not the iterate
    size_t packed_frame_bytes;                // nine-point: bytes of one packed frame (the extra term of its persistent-form test)
    int persist_chunks;                       // nine-point: pde8_persist_chunks(nrows); 0: the five-point walkers' count
};
// PDEIP_* of the environment (read_sor_knobs).
struct SorKnobs {
    bool persist = true, walk = false, small = true, fuse = true, pipe = true;
    int small_q = 1, rb_tj = 0, rbp_tj = 0, serpentine = 0; // serpentine -1: PDEIP_RBP_SERPENTINE absent, the frame decides
};
// cus: compute units; rb2_slots: resident waves of the two-sweep march; rbp_slots: resident workgroups of k_sor_rbp.  A fact that is
// 0 is not known yet: the planner asks for it -- ask(FACT_*) returns it -- only where the call's path needs it, as a call always has
// (a call that k_sor_small serves in one slab asks nothing).
struct SorDevice { int cus, rb2_slots, rbp_slots; };
enum { FACT_CUS, FACT_RB2, FACT_RBP };

// One launch; in SorPlan::step, `count` launches of the same shape (first, src and dst are set by for_each_launch).
struct SorLaunch { int kind, sweeps, first, tj, tiles, units, gridx, src, dst, count, index; };
struct SorPlan {
    int family = SOR_NONE, form = FORM_NONE;
    int A = 0, B = 0, NC = 0, W = 0, last_m = 0; // exact order: row tiles, strips of W columns, chunks per strip, the last front
    int nsteps = 0, nlaunch = 0;                 // nlaunch: what pdeip_last_launch_count() reports
    SorLaunch step[4] = {};
    bool has_dst = false, vec = false;
    int mirror_mode = 0;        // k_sor_rbp: PDEIP_RBP_SERPENTINE, 0..3; what a launch runs with is resolve_mirror()'s answer
    bool copy_in = false;       // the caller's iterate is copied to the destination first (exact order relaxes there; iter <= 0)
    bool copy_back = false;     // in place and the last launch wrote the scratch copy
    bool persist_setup = false; // k_persist_setup runs in front of the walker (not counted)
    SmallPlan small;
    void add(int kind, int count, int sweeps = 0, int tj = 0, int tiles = 0, int units = 0, int gridx = 0)
    {
        if (count <= 0) return;
        step[nsteps++] = SorLaunch{kind, sweeps, 0, tj, tiles, units, gridx, 0, 0, count, 0};
        nlaunch += count;
    }
};

// Reads one set of knobs into k: a call reads the set of the path it takes, when it takes it (a call that k_sor_small serves never
// looks at the strip widths, one that launches no k_sor_rbp never at the pipeline's).  PDEIP_RB_FUSE is read once per process,
// the others per call: the tests switch them.
enum { KNOBS_EXACT, KNOBS_SMALL, KNOBS_CHAIN, KNOBS_PIPE };
inline void read_sor_knobs(SorKnobs &k, int set, bool pde8 = false)
{
    if (set == KNOBS_EXACT) {
        k.persist = env_int(pde8 ? "PDEIP_PDE8_PERSIST" : "PDEIP_EXACT_PERSIST", 1) != 0; // 0: one launch per front
        k.walk = !pde8 && k.persist && env_int("PDEIP_EXACT_WALK", 0) != 0;               // opt-in: pdeip_sor_walk.hpp
    } else if (set == KNOBS_SMALL) {
        k.small = env_int("PDEIP_RB_SMALL", 1) != 0;
        if (k.small) k.small_q = env_int("PDEIP_SMALL_Q", 1); // 1 measured fastest at every scale (tools/time_small.py)
    } else if (set == KNOBS_CHAIN) {
        static const bool fuse_enabled = env_int("PDEIP_RB_FUSE", 1) != 0; // two sweeps per launch; 0 keeps one sweep per launch
        k.fuse = fuse_enabled;
        k.rb_tj = g.rb_tj > 0 ? g.rb_tj : env_int("PDEIP_RB_TJ", 0);
        k.pipe = !pde8 && env_int("PDEIP_RB_PIPE", 1) != 0;
    } else { // a call that launches the pipeline
        k.rbp_tj = env_int("PDEIP_RBP_TJ", 0);
        // 1: alternate strips march backwards (k_sor_rbp, `mirror_mode`), 2: every strip (tests).  Same bits; at 4K the launch is
        // not faster for the halo columns neighbours then share (97.7 vs 94.6 us): the pipeline's step sets its time.
        // 3: alternate whole LAUNCHES (resolve_mirror).  A launch ends at the east end of every strip, and those are the lines the
        // Infinity Cache holds when the next launch -- of this call or of the next one -- begins: marched east -> west it starts on
        // hits instead of evicting them before it gets there.  Elin4 4K, iter = 4 per call: 98.3 -> 84.8 and 95.2 -> 85.0 us per
        // step on two devices (tools/time_rbp_alternate.py, profiles/NOTES.md R6.1).  A value that is present is obeyed as it
        // stands; absent (-1 here), the frame decides (default_mirror).
        const char *serp = getenv("PDEIP_RBP_SERPENTINE");
        const bool set = serp && *serp;
        const int v = set ? atoi(serp) : 0;
        k.serpentine = !set ? -1 : (v < 0 || v > MIRROR_ALTERNATE ? 0 : v);
    }
}

// The persistent exact-order forms pack strip, sweep and column into 16-bit fields and address a frame's planes with 32 bits.
inline bool persist_fits(int strips, int iter, size_t plane_bytes, int ncols)
{
    return strips <= 0xffff && iter <= 0x7fff && plane_bytes < 0xffff0000ull && ncols <= 65535;
}

// Columns per unit of the one-sweep red-black kernels.  Narrow strips mean more waves in flight but more halo re-reads
// ((TJ+2)/TJ coefficient, (TJ+4)/TJ iterate columns).  12 is the measured optimum at 4K (2880 units) and at 1080p; a strip stride
// that is a multiple of a large power of two aliases on HBM channels (TJ=16 at nrows=2160 is 15 % slower than 12).
inline int pick_rb_tj(int forced) { return forced > 0 ? (forced < 2 ? 2 : forced) : 12; }

// Strip width of the two-sweeps-per-launch kernels.  They hold four column stages in registers (one wave per SIMD) and are bound
// by their instruction stream, not by HBM: a launch takes ceil(units / resident waves) rounds of (TJ + 6) steps, so the best TJ
// is the one that fills the last round (4K: 12 -> 3 rounds of 18 steps, 133 us; 34 -> 1 round of 40 steps, 113 us; 33 -> 2 rounds).
inline int pick_rb2_tj(int slots, int tiles, int ncols, int nframes)
{
    int best = 12;
    long best_cost = -1;
    for (int tj = 2; tj <= 64; tj++) {
        const long units = (long)tiles * ((ncols + tj - 1) / tj) * nframes;
        const long cost = ((units + slots - 1) / slots) * (tj + 6);
        if (best_cost < 0 || cost <= best_cost) { // ties: the wider strip re-reads fewer halo columns
            best_cost = cost;
            best = tj;
        }
    }
    return best;
}

// Strip width of the pipelined kernel (pdeip_sor_rbp.hpp): one workgroup per CU, a launch takes ceil(units / resident
// workgroups) rounds of nsteps(TJ) = TJ + 5S - 1 steps.
inline int pick_rbp_tj(int slots, int tiles, int ncols, int nframes, int tail)
{
    int best = 64;
    long best_cost = -1;
    for (int tj = 8; tj <= 1024; tj++) {
        const long units = (long)tiles * ((ncols + tj - 1) / tj) * nframes;
        const long cost = ((units + slots - 1) / slots) * (tj + tail);
        if (best_cost < 0 || cost < best_cost) {
            best_cost = cost;
            best = tj;
        }
    }
    return best;
}

// Exact order.  Launch-per-front or persistent?  The persistent form wins at every iter and frame size
// (tools/time_exact_persist.py: 4K 2.70 vs 2.87 ms at iter=4, 1.4x at iter=20, 1.3x at 1080p, 2.4x at 34x60: no per-front launch,
// sweeps overlap more tightly).  The walker (LDS-DMA loader, strips of W columns) is 15 % faster at 4K with one sweep per call,
// 2-5 % at iter = 4 and 5-25 % SLOWER below 1080p and for the single-field models: opt-in (exact order).
inline void plan_exact(SorPlan &p, const SorTraits &t, const SorShape &sh, const SorKnobs &k)
{
    const int skew = t.ex_skew;
    const int b64 = (sh.ncols - 2 + 63) / 64;
    const size_t n = (size_t)sh.nrows * sh.ncols;
    p.family = SOR_EXACT;
    p.copy_in = sh.has_dst;
    p.A = (sh.nrows - 2 + skew * 63 + EX_R - 1) / EX_R;
    p.last_m = (p.A - 1) + (skew + 1) * (b64 - 1) + (skew + 2) * (sh.iter - 1);
    const bool persist = k.persist && persist_fits(b64, sh.iter, n * (t.pde8 ? 1 : t.ncf) * sizeof(float), sh.ncols) && sh.packed_frame_bytes < 0xffff0000ull;
    p.W = persist && k.walk ? t.walk_width(sh.nrows, sh.ncols, sh.nframes, sh.iter) : 64;
    p.B = (sh.ncols - 2 + p.W - 1) / p.W;
    if (persist) {
        p.form = k.walk ? FORM_WALK : FORM_PERSIST;
        p.NC = sh.persist_chunks > 0 ? sh.persist_chunks : (sh.nrows - 2 + 63 + EX_CH - 1) / EX_CH;
        p.persist_setup = true;
        p.add(K_PACK, 1);
        p.add(k.walk ? K_WALK : K_PERSIST, 1, sh.iter, p.W, p.NC, p.B, p.B * sh.iter * sh.nframes);
    } else {
        p.form = FORM_FRONT;
        p.add(K_DERIVE, 1);
        p.add(K_FRONT, p.last_m + 1, 0, 64, p.A, p.B, p.B * sh.iter);
    }
    p.add(K_BORDERS, 1);
}

// Small frames: the iterate resident in LDS, one launch per (up to) four sweeps (pdeip_sor_small.hpp).  A cut frame relaxed in
// place needs every workgroup resident at once (its load counter): at most one workgroup per compute unit, with an eighth of
// the device left for whatever else is running.
template <class Ask> inline bool plan_small(SorPlan &p, const SorTraits &t, const SorShape &sh, const SorKnobs &k, int cus, Ask &&ask)
{
    const int q = k.small_q < 1 ? 1 : k.small_q;
    SmallPlan sp = t.small(sh.nrows, sh.ncols, sh.iter, q);
    int per_launch = sh.iter;
    if (!sp.ok && sh.iter > SMALL_MAX_SWEEPS) {
        sp = t.small(sh.nrows, sh.ncols, SMALL_MAX_SWEEPS, q);
        per_launch = SMALL_MAX_SWEEPS;
    }
    if (sp.ok && sp.nslabs > 1 && cus <= 0) cus = ask(FACT_CUS);
    if (!sp.ok || (sp.nslabs > 1 && (long)sp.nslabs * sh.nframes > (long)cus - cus / 8)) return false;
    p.family = SOR_SMALL;
    p.small = sp;
    p.add(K_SMALL, sh.iter / per_launch, per_launch, sp.W, 1, sp.nslabs, sp.nslabs);
    p.add(K_SMALL, sh.iter % per_launch ? 1 : 0, sh.iter % per_launch, sp.W, 1, sp.nslabs, sp.nslabs);
    return true;
}

// Red-black (four-colour for the nine-point model): launches that ping-pong between the caller's buffers and a scratch copy.
// Four sweeps per launch where the rings fit in LDS (pdeip_sor_rbp.hpp; PDEIP_RB_PIPE=0 disables it), two where the model allows
// it (rb_march2: same results, about two thirds of the traffic per sweep), one for an odd sweep left over.
template <class Ask> inline void plan_chain(SorPlan &p, const SorTraits &t, const SorShape &sh, SorKnobs &k, const SorDevice &dev, Ask &&ask)
{
    const size_t n = (size_t)sh.nrows * sh.ncols;
    const auto strips = [&](int tj) { return (sh.ncols + tj - 1) / tj; };
    p.vec = sh.nrows % 4 == 0 && sh.aligned16;
    // single-field models run one wave per sweep (one wave per SIMD): the pipeline only pays on large frames there
    const bool pipe = k.pipe && k.fuse && p.vec && t.rbp_fits && (t.rbp_nw == 2 || n >= (size_t)1 << 21);
    const int n4 = pipe ? sh.iter / RBP_SWEEPS : 0, rest = sh.iter - RBP_SWEEPS * n4, n2 = k.fuse ? rest / 2 : 0, n1 = rest - 2 * n2;
    p.family = t.pde8 ? SOR_PDE8 : (n4 > 0 ? SOR_RBP : SOR_RB);
    if (n4 > 0) {
        read_sor_knobs(k, KNOBS_PIPE);
        const int tiles = (sh.nrows + t.rbp_own - 1) / t.rbp_own;
        const int tj = k.rbp_tj > 0 ? (k.rbp_tj < 2 ? 2 : k.rbp_tj)
                                    : pick_rbp_tj(dev.rbp_slots > 0 ? dev.rbp_slots : ask(FACT_RBP), tiles, sh.ncols, sh.nframes, t.rbp_tail);
        p.add(K_RBP, n4, RBP_SWEEPS, tj, tiles, tiles * strips(tj), tiles * strips(tj));
    }
    const int tj1 = pick_rb_tj(k.rb_tj), tiles1 = rb_row_tiles(sh.nrows, RB_OWN_ROWS), tiles2 = rb_row_tiles(sh.nrows, t.rb2_own);
    const int tj2 = (k.rb_tj > 0 || n2 == 0) ? tj1 : pick_rb2_tj(dev.rb2_slots > 0 ? dev.rb2_slots : ask(FACT_RB2), tiles2, sh.ncols, sh.nframes);
    const auto blocks = [](int units) { return (units + RB_WAVES_PER_BLOCK - 1) / RB_WAVES_PER_BLOCK; };
    p.add(t.pde8 ? K_P8C2 : K_RB2, n2, 2, tj2, tiles2, tiles2 * strips(tj2), blocks(tiles2 * strips(tj2)));
    p.add(t.pde8 ? K_P8C1 : K_RB1, n1, 1, tj1, tiles1, tiles1 * strips(tj1), blocks(tiles1 * strips(tj1)));
    p.copy_back = !sh.has_dst && (p.nlaunch & 1);
}

// The mirror mode of a call that does not set PDEIP_RBP_SERPENTINE: launches alternate (3) where the planes of a launch -- thirteen
// for the flow model the rule was measured on, 13 * pixels * frames * 4 bytes -- exceed the 256 MiB of the Infinity Cache, and all
// march forwards (0) below.  Where everything stays resident between launches there is nothing to win back, and a mirrored launch
// by itself was up to 3 % slower than a forward one at 1080p (33.2 vs 32.3 us on one of two devices: NOTES R6.1).
inline int default_mirror(const SorShape &sh)
{
    return (size_t)13 * sh.nrows * sh.ncols * sh.nframes * sizeof(float) > ((size_t)256 << 20) ? MIRROR_ALTERNATE : 0;
}

// The planner reads the knobs (and nothing else outside its arguments) and makes no HIP call; `ask` may.
template <class Ask> inline SorPlan plan_sor(const SorTraits &t, const SorShape &sh, const SorDevice &dev, Ask &&ask)
{
    SorPlan p;
    SorKnobs k;
    p.has_dst = sh.has_dst;
    if (sh.iter <= 0) {
        p.copy_in = sh.has_dst; // a copy, nothing else
    } else if (sh.mode != PDEIP_MODE_RED_BLACK) { // LINE_SCAN only changes line relaxation
        read_sor_knobs(k, KNOBS_EXACT, t.pde8);
        plan_exact(p, t, sh, k);
    } else {
        if (!t.pde8) read_sor_knobs(k, KNOBS_SMALL);
        if (t.pde8 || !k.small || !plan_small(p, t, sh, k, dev.cus, ask)) {
            read_sor_knobs(k, KNOBS_CHAIN, t.pde8);
            plan_chain(p, t, sh, k, dev, ask);
            p.mirror_mode = k.serpentine >= 0 ? k.serpentine : default_mirror(sh);
        }
    }
    return p;
}

// The mirror mode one k_sor_rbp launch runs with (0, 1 or 2), from the plan's mode and the device's bit (DeviceState::rbp_next_mirror),
// set while the device's last pipeline launch ended at the east ends of its strips.  Mode 3 mirrors the launch when the bit is
// set; modes 0 .. 2 are obeyed as they stand.  Either way the bit then says where THIS launch ends (mode 1, half the strips
// each way, counts as forward), so under mode 3 it flips with every launch: launches 2, 3, ... of a call and the first launch
// of the next call each start where the one before ended.  Every direction gives the same bits (pdeip_sor_rbp.hpp), so neither
// the bit's history nor a direction frozen into a captured graph can change a result.
inline int resolve_mirror(int mode, bool &next_mirror)
{
    const int m = mode == MIRROR_ALTERNATE ? (next_mirror ? 2 : 0) : mode;
    next_mirror = m != 2;
    return m;
}

// Calls fn(launch) for every launch of the plan, in order.  Launch i of a ping-pong chain reads what launch i - 1 wrote.  In
// place: caller <-> scratch.  With a destination the caller's buffers are only read, by launch 0, and the outputs alternate so
// that the last one is the destination.  Exact order and k_sor_small work on one buffer (after launch 0, for k_sor_small).
template <class F> inline int for_each_launch(const SorPlan &p, F &&fn)
{
    const int home = p.has_dst ? BUF_DST : BUF_CALLER;
    const auto out = [&](int i) -> int {
        if (p.family < SOR_RB) return home;
        if (p.has_dst) return ((p.nlaunch - 1 - i) & 1) ? BUF_SCRATCH : BUF_DST;
        return (i & 1) ? BUF_CALLER : BUF_SCRATCH;
    };
    int i = 0;
    for (int s = 0; s < p.nsteps; s++)
        for (int c = 0; c < p.step[s].count; c++, i++) {
            SorLaunch l = p.step[s];
            l.index = i;
            l.first = p.family != SOR_EXACT && i == 0; // the launch that finds raw planes in the derived slots
            l.src = (i == 0 && p.family != SOR_EXACT) ? BUF_CALLER : out(i - 1);
            l.dst = out(i);
            RC(fn(l));
        }
    return PDEIP_OK;
}

// The nine-point model's plan (pdeip_sor9.hip: its kernels and layouts live in that unit).  A fact of `dev` that is 0 and that the
// call needs is asked from the current device.
SorPlan plan_sor_pde8(SorShape sh, const SorDevice &dev);

} // namespace pdeip
