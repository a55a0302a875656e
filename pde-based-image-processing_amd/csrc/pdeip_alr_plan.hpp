// pdeip_alr_plan.hpp -- alternating line relaxation: what a call launches, decided before the first launch.
//
// plan_alr() turns two facts about the model, the call's shape and the knobs it asks for into an AlrPlan: the family, the launches in front
// of the iterations, one pass record per direction, the workspace the call fetches and its launch count.  Plain C++ (no HIP, no
// library state): run_alr (pdeip_line.hip) registers the call's planes, plans, fetches the workspace and loops over the plan;
// pdeip_debug_plan_alr() answers on a machine without a GPU (tests/test_alr_plan.py compares it with tests/seam_model.py and
// tests/line_scan_cases.py).  The constants the decision needs are stated here, once; pdeip_alr.hpp includes this header.
#pragma once
#include <cstddef>

#include "../../include/pdeip.h"

#ifdef __HIPCC__
#define PDEIP_ALR_HD __host__ __device__
#else
#define PDEIP_ALR_HD
#endif

namespace pdeip {

constexpr int ALR_TB_MAX = 16;                     // planes per launch of k_alr_transpose_batch
constexpr int ALR_SMALL_THREADS = 1024;            // k_alr_small: one workgroup per frame
constexpr int ALR_SMALL_MAXTR = 24;                // coefficient planes its argument block holds
// one CU evaluates every row of the call: worth it where a pass is a few microseconds of work, i.e. up to ~60 x 100
// (tools/time_alr_small.py: 34x60 348 -> 161 us, 17x30 294 -> 94 us, 61x108 407 -> 367 us, 68x120 392 -> 434 us)
constexpr long ALR_SMALL_MAX_PIXELS = 6144;
constexpr size_t ALR_SMALL_MAX_LDS = 150 * 1024;   // and its largest colour pass fits this much LDS
constexpr int ZB_NM = 7;                           // k_alr_zebra3: mover waves = tiles per round
constexpr int ZB_LW = 8;                           // lines per workgroup
constexpr int ZB_TE = 32;                          // elements per tile
constexpr int ZB_THREADS = 64 * (1 + ZB_NM);
constexpr int Z3_LSF = 3 * ZB_TE + 4;              // floats per line of a tile; +4 keeps the 16 lines' b128 reads on distinct banks
constexpr int Z3_TILE = ZB_LW * Z3_LSF;            // floats per tile
constexpr size_t Z3_LDS_BYTES = (size_t)2 * ZB_NM * Z3_TILE * sizeof(float);
constexpr int ALR_LEX_THREADS = 1024;
constexpr int ALR_SCAN_THREADS = ALR_LEX_THREADS;
constexpr int ALR_SCAN_VEC = 4;                    // elements per group: one coef4
constexpr int ALR_SCAN_MAXG = 3;                   // groups per lane at most: lines of up to 12 288 elements (6 144 for each of two coupled fields)
constexpr size_t ALR_LINE_ELEM = 16;               // k_alr_lex holds a line as one float4 per element
constexpr size_t ALR_LINE_BUDGET = 160 * 1024;     // LDS its line buffers may take
constexpr size_t ALR_LDS_OPT_IN = 64 * 1024;       // dynamic LDS beyond this needs ensure_lds

// LDS of k_alr_small per colour pass: a row (a, divisor, cp, d) and the old / new x of every element of the colour's lines; lines
// padded to an odd number of rows so that the lanes of the recurrence stage (one per line) hit different banks
PDEIP_ALR_HD inline int alr_small_stride(int n) { return n | 1; }
PDEIP_ALR_HD inline size_t alr_small_elems(int nrows, int ncols, bool interior_lines)
{
    const int lo = interior_lines ? 1 : 0;
    const size_t col_lines = (size_t)(ncols - 2 * lo + 1) / 2, row_lines = (size_t)(nrows - 2 * lo + 1) / 2;
    const size_t a = col_lines * (size_t)alr_small_stride(nrows), b = row_lines * (size_t)alr_small_stride(ncols);
    return a > b ? a : b;
}
inline size_t alr_small_lds_bytes(int nrows, int ncols, bool interior_lines) { return alr_small_elems(nrows, ncols, interior_lines) * (ALR_LINE_ELEM + sizeof(float)); }

enum { ALR_NONE = 0, ALR_SMALL, ALR_ZEBRA, ALR_EXACT, ALR_SCAN };             // family (ALR_NONE: nothing to do)
enum { AK_ZEBRA3 = 1, AK_ZEBRA3_PAIR, AK_LEX, AK_LEX_GLOBAL, AK_SCAN };       // kernel of a pass (AK_LEX_GLOBAL: k_alr_lex<GL = true>)

struct AlrTraits {
    int chains;          // fields the model's solver couples (ALR_MODEL_CHAINS)
    bool interior_lines; // Mdl::INTERIOR_LINES
};
struct AlrShape {
    int nrows, ncols, nframes, iter, mode, nch;
    int nplanes, ncoef; // distinct planes of the call, and those of them that are no iterate
};
// PDEIP_ALR_* of the environment, env(name, default).  Each is read per call (the tests switch them) and only when the plan asks
// for it, that is on the path that uses it.
template <class Env> struct AlrKnobs {
    Env env;
    bool small() const { return env("PDEIP_ALR_SMALL", 1) != 0; } // 0: no k_alr_small (asked of a zebra call)
    bool pair() const { return env("PDEIP_ALR_PAIR", 1) != 0; }   // 0: one zebra launch per field and colour (a zebra call of two fields)
    bool scan() const { return env("PDEIP_ALR_SCAN", 1) != 0; }   // 0: the exact-order kernel everywhere (a LINE_SCAN call)
};
template <class Env> inline AlrKnobs<Env> alr_knobs(Env env) { return AlrKnobs<Env>{env}; }

struct AlrColour { int first, last, gridx; }; // lines first, first + 2, ... last of one zebra launch
// One direction of an iteration ([0] along the columns, [1] along the rows).
struct AlrPass {
    int kind = 0;
    int lo = 0, hi = 0, n = 0;   // lines lo..hi of n elements
    int factor_gridx = 0;        // grid x of the factor launch over all of them
    int ncolours = 0;            // zebra: a colour without a line is left out
    AlrColour colour[2] = {};
    int chains = 0, launches = 0; // chains per launch, launches per pass
    int G = 0;                   // k_alr_scan: groups of ALR_SCAN_VEC elements per lane
    size_t lds = 0;              // dynamic LDS bytes of a launch
    bool opt_in = false;         // ... which need the opt-in
    int gridx = 0;               // exact order and scan: one workgroup per frame
    int order[2] = {0, 0};       // the call's fields in the order the pass takes them
};
struct AlrPlan {
    int family = ALR_NONE;
    int coef_transposes = 0;     // k_alr_transpose_batch launches for the coefficient planes (0: k_alr_small transposes them itself)
    int factor_launches = 0;     // k_alr_factor_pair: 2; k_alr_zebra3<ZB_FACTOR>: 2 per chain
    bool factor_pair = false;
    int iterate_transposes = 0;  // per iteration
    AlrPass pass[2];
    size_t small_lds = 0;        // k_alr_small
    bool small_opt_in = false;
    size_t ws_alr = 0, ws_alr_t = 0, ws_aux1 = 0, ws_lex = 0; // floats of each workspace slot the call fetches
    int nlaunch = 0;             // what pdeip_last_launch_count() reports
};

// Does k_alr_lex hold a line of n elements in LDS for `chains` fields at once?  Two coupled fields: up to 5120 elements; one: 10240.
inline bool alr_lines_fit(int chains, int n) { return (size_t)chains * (size_t)n * ALR_LINE_ELEM <= ALR_LINE_BUDGET; }
// The scan kernels take every line that passes that test.
static_assert(ALR_LINE_BUDGET / ALR_LINE_ELEM <= (size_t)ALR_SCAN_MAXG * ALR_SCAN_THREADS * ALR_SCAN_VEC, "k_alr_scan: groups per lane");

// zebra order on a small frame: the whole call in one launch (k_alr_small)
inline bool alr_small_admits(const AlrTraits &t, const AlrShape &sh)
{
    return alr_small_lds_bytes(sh.nrows, sh.ncols, t.interior_lines) <= ALR_SMALL_MAX_LDS && sh.nrows >= 3 && sh.ncols >= 3 &&
           (long)sh.nrows * sh.ncols <= ALR_SMALL_MAX_PIXELS && sh.ncoef <= ALR_SMALL_MAXTR;
}

template <class Knobs> inline AlrPlan plan_alr(const AlrTraits &t, const AlrShape &sh, const Knobs &k)
{
    AlrPlan p;
    if (sh.iter <= 0) return p;
    const size_t plane = (size_t)sh.nrows * sh.ncols * sh.nframes;
    const int lo = t.interior_lines ? 1 : 0, longest = sh.nrows > sh.ncols ? sh.nrows : sh.ncols;
    const bool zebra = sh.mode == PDEIP_MODE_RED_BLACK;
    p.ws_alr = plane * 8;                              // cp and divisor plane per (field, direction)
    p.ws_alr_t = plane * (size_t)sh.nplanes;            // a transposed twin of every plane
    if (zebra && k.small() && alr_small_admits(t, sh)) {
        p.family = ALR_SMALL;
        p.small_lds = alr_small_lds_bytes(sh.nrows, sh.ncols, t.interior_lines);
        p.small_opt_in = p.small_lds > ALR_LDS_OPT_IN;
        p.nlaunch = 1;
        return p;
    }
    // LINE_SCAN: a line's recurrences as scans (k_alr_scan).  A call whose longer lines k_alr_lex could not hold in LDS for all
    // chains at once takes the exact-order kernels in both directions, as EXACT_ORDER does: bit-exact, hence inside the contract.
    const bool scan = sh.mode == PDEIP_MODE_LINE_SCAN && k.scan() && sh.nch == t.chains && alr_lines_fit(sh.nch, longest);
    const bool pair = zebra && sh.nch == 2 && k.pair(); // both fields of a coupled solver in one launch per colour
    p.family = zebra ? ALR_ZEBRA : (scan ? ALR_SCAN : ALR_EXACT);
    p.coef_transposes = (sh.ncoef + ALR_TB_MAX - 1) / ALR_TB_MAX;
    p.factor_pair = sh.nch == 2;
    p.factor_launches = p.factor_pair ? 2 : 2 * sh.nch;
    p.iterate_transposes = 2;
    if (zebra) p.ws_aux1 = plane; // dp of the lines in flight
    for (int d = 0; d < 2; d++) {
        AlrPass &q = p.pass[d];
        q.lo = lo;
        q.hi = (d == 0 ? sh.ncols : sh.nrows) - 1 - lo;
        q.n = d == 0 ? sh.nrows : sh.ncols;
        q.factor_gridx = (q.hi - lo + 1 + ZB_LW - 1) / ZB_LW;
        // the reference relaxes columns of field 0 then field 1, rows of field 1 then field 0 (opticalflowSolvers.c:231-258)
        q.order[0] = (d == 1 && sh.nch == 2) ? 1 : 0;
        q.order[1] = 1 - q.order[0];
        q.gridx = sh.nframes;
        if (zebra) {
            q.kind = pair ? AK_ZEBRA3_PAIR : AK_ZEBRA3;
            q.chains = pair ? 2 : 1;
            q.lds = Z3_LDS_BYTES;
            for (int colour = 0; colour < 2; colour++) {
                const int first = lo + (((lo & 1) != colour) ? 1 : 0);
                if (first > q.hi) continue;
                const int last = q.hi - (((q.hi & 1) != colour) ? 1 : 0), count = (last - first) / 2 + 1;
                q.colour[q.ncolours++] = AlrColour{first, last, (count + ZB_LW - 1) / ZB_LW};
            }
            q.launches = q.ncolours * sh.nch / q.chains;
            q.gridx = 0;
        } else if (scan) {
            const int per_group = ALR_SCAN_THREADS / sh.nch * ALR_SCAN_VEC; // the chains share the workgroup's threads
            q.kind = AK_SCAN;
            q.chains = sh.nch;
            q.launches = 1;
            q.G = q.n <= per_group ? 1 : (q.n + per_group - 1) / per_group;
        } else if (!alr_lines_fit(1, q.n)) { // the line buffer in global memory, one chain per launch (correct, slow)
            q.kind = AK_LEX_GLOBAL;
            q.chains = 1;
            q.launches = sh.nch;
            const size_t need = (size_t)q.n * (ALR_LINE_ELEM / sizeof(float)) * sh.nframes;
            if (need > p.ws_lex) p.ws_lex = need;
        } else {
            q.kind = AK_LEX;
            q.chains = sh.nch == 2 && alr_lines_fit(2, q.n) ? 2 : 1; // chain 1 trails chain 0 by a line
            q.launches = sh.nch / q.chains;
            q.lds = (size_t)q.chains * q.n * ALR_LINE_ELEM;
        }
        q.opt_in = q.lds > ALR_LDS_OPT_IN;
    }
    p.nlaunch = p.coef_transposes + p.factor_launches + sh.iter * (p.pass[0].launches + p.pass[1].launches + p.iterate_transposes);
    return p;
}

} // namespace pdeip
