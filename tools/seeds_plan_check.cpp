// seeds_plan_check.cpp -- the host-side decisions of generateSeeds() and the dense driver (csrc/pdeip_seeds_plan.hpp: argument
// checks, scale sizes, visit order, the RITER / RCONS schedule, the consensus-set vector, stage seeds) exercised on their own, for
// the host sanitizers:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/seeds_plan_check.cpp -o seeds_plan_check && ./seeds_plan_check
//
// No HIP and no GPU: nothing here is loaded into another process.  Exit status 0 and "ok" on success.
#include "../pde-based-image-processing_amd/csrc/pdeip_seeds_plan.hpp"

#include <climits>
#include <cstring>

using namespace pdeip::seeds;

static int failures = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("%s:%d: %s is false\n", __FILE__, __LINE__, #cond); \
            failures++;                                                    \
        }                                                                  \
    } while (0)

static const double CS[3] = {0.1, 0.4, 0.7};

static bool refused(const char *word, int nr, int nc, int order, double sig, const double *cs, int ncs, int it, int sd, double f, double ps)
{
    char buf[160];
    const char *m = check_args(buf, sizeof buf, nr, nc, order, sig, cs, ncs, it, sd, f, ps);
    return m != nullptr && std::strstr(m, word) != nullptr;
}

int main()
{
    char buf[160];
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    EXPECT(check_args(buf, sizeof buf, 3, 3, 1, 0.7, CS, 3, 0, 1, 0.7, 0.2) == nullptr);
    EXPECT(check_args(buf, sizeof buf, 288, 384, 2, 1.2, CS, 1, 20, 15, 0.7, 0.4) == nullptr);
    EXPECT(check_args(buf, sizeof buf, 2160, 3840, 2, 1.2, CS, 3, 20, 15, 0.999, 5.0) == nullptr);
    EXPECT(refused("3x3", 2, 8, 1, 0.7, CS, 3, 3, 2, 0.7, 0.4));
    EXPECT(refused("3x3", 8, INT_MIN, 1, 0.7, CS, 3, 3, 2, 0.7, 0.4));
    EXPECT(refused("seeds", 8, 8, 1, 0.7, CS, 3, 3, 0, 0.7, 0.4));
    EXPECT(refused("seeds", 8, 8, 1, 0.7, CS, 3, 3, INT_MAX, 0.7, 0.4));
    EXPECT(refused("too large", INT_MAX, INT_MAX, 1, 0.7, CS, 3, 3, 65535, 0.7, 0.4));
    EXPECT(refused("too large", 4096, 4096, 1, 0.7, CS, 3, 3, 65535, 0.7, 0.4));
    EXPECT(refused("iterations", 8, 8, 1, 0.7, CS, 3, INT_MIN, 2, 0.7, 0.4));
    for (int order : {INT_MIN, 0, 3, INT_MAX}) EXPECT(refused("order", 8, 8, order, 0.7, CS, 3, 3, 2, 0.7, 0.4));
    for (double s : {nan, inf, -inf, 0.0, -1.0}) EXPECT(refused("sigmaLim", 8, 8, 1, s, CS, 3, 3, 2, 0.7, 0.4));
    EXPECT(refused("cset_vect", 8, 8, 1, 0.7, nullptr, 3, 3, 2, 0.7, 0.4));
    EXPECT(refused("cset_vect", 8, 8, 1, 0.7, CS, 0, 3, 2, 0.7, 0.4));
    EXPECT(refused("cset_vect", 8, 8, 1, 0.7, CS, INT_MIN, 3, 2, 0.7, 0.4));
    {
        const double bad[3] = {0.1, 0.2, nan};
        EXPECT(refused("cset_vect[2]", 8, 8, 1, 0.7, bad, 3, 3, 2, 0.7, 0.4));
        EXPECT(check_args(buf, sizeof buf, 8, 8, 1, 0.7, bad, 2, 3, 2, 0.7, 0.4) == nullptr); // the entry beyond n_cset is not read
    }
    for (double f : {nan, 0.0, 1.0, -0.5, inf}) EXPECT(refused("scl_factor", 8, 8, 1, 0.7, CS, 3, 3, 2, f, 0.4));
    for (double p : {nan, 0.0, -0.5, inf}) EXPECT(refused("pyr_scl", 8, 8, 1, 0.7, CS, 3, 3, 2, 0.7, p));

    // the scale sizes the drivers meet: 288x384 with gen_scl 0.2 and rc_scl 0.4, the tests' 60x80, extremes that must terminate
    {
        const std::vector<Size> g = scale_sizes(288, 384, 0.7, 0.2);
        EXPECT(g.size() == 5 && g[1].r == 202 && g[1].c == 269 && g[4].r == 70 && g[4].c == 94);
        const std::vector<Size> r = scale_sizes(288, 384, 0.7, 0.4);
        EXPECT(r.size() == 3 && r[2].r == 142 && r[2].c == 189);
        const std::vector<Size> t = scale_sizes(60, 80, 0.7, 0.4);
        EXPECT(t.size() == 3 && t[1].r == 42 && t[1].c == 56 && t[2].r == 30 && t[2].c == 40);
        EXPECT(scale_sizes(60, 80, 0.3, 0.2).size() == 2);
    }
    for (int nr : {3, 4, 37, 60, 288, 2160, 46340})
        for (int nc : {3, 5, 53, 80, 384, 3840})
            for (double f : {1e-9, 0.3, 0.5, 0.7, 0.99, 0.999999999})
                for (double ps : {1e-9, 0.2, 0.4, 1.0, 7.0}) {
                    const std::vector<Size> sz = scale_sizes(nr, nc, f, ps);
                    EXPECT(!sz.empty() && sz[0].r == nr && sz[0].c == nc && sz.size() < 4000);
                    for (size_t k = 1; k < sz.size(); k++) {
                        EXPECT(sz[k].r >= 3 && sz[k].c >= 3 && sz[k].r <= sz[k - 1].r && sz[k].c <= sz[k - 1].c);
                        EXPECT(sz[k].r < sz[k - 1].r || sz[k].c < sz[k - 1].c);
                        EXPECT((double)sz[k].r >= nr * ps && (double)sz[k].c >= nc * ps);
                    }
                    const int K = (int)sz.size();
                    std::vector<int> seen((size_t)K, 0);
                    for (int v = 0; v < 2 * K; v++) {
                        const int k = visit_scale(v, K);
                        EXPECT(k >= 0 && k < K);
                        seen[(size_t)k]++;
                    }
                    for (int k = 0; k < K; k++) EXPECT(seen[(size_t)k] == 2);
                    EXPECT(visit_scale(0, K) == 0 && visit_scale(K - 1, K) == K - 1 && visit_scale(K, K) == K - 1 && visit_scale(2 * K - 1, K) == 0);
                }

    // RITER / RCONS: every (iteration, visit) reads inside cset_vect, also with a vector shorter than the iterations
    for (int n = 1; n <= 12; n++) {
        std::vector<double> cs((size_t)n);
        for (int i = 0; i < n; i++) cs[(size_t)i] = 0.1 + 0.01 * i;
        for (int v = 0; v < 8; v++)
            for (int it = 1; it <= 40; it++) {
                const double want = v == 0 ? cs[(size_t)((it < n ? it : n) - 1)] : cs[(size_t)n - 1];
                EXPECT(rcons(cs.data(), n, it, v) == want);
                EXPECT(riter(it, v) == ((it == 1 && v == 0) ? 2000 : 100));
            }
        EXPECT(rcons(cs.data(), n, INT_MAX, 0) == cs[(size_t)n - 1]);
    }
    EXPECT(nu_of(0.01, 60, 80) == (float)(0.01 * std::pow(4800.0, 0.7)));
    EXPECT(nu_of(0.01, 46340, 46340) > 0.0f);

    // the constants: NaN members keep the dense values
    {
        const Prm d = resolve(nullptr, nullptr, nullptr);
        EXPECT(d.dist_cap == inf && d.mincov_gate == -inf && std::isnan(d.nan_fill));
        const double cap = 100.0, fill = 1000.0, gate = 0.5;
        const Prm s = resolve(&cap, &fill, &gate);
        EXPECT(s.dist_cap == 100.0 && s.nan_fill == 1000.0f && s.mincov_gate == 0.5);
        const Prm m = resolve(&nan, &fill, &nan);
        EXPECT(m.dist_cap == inf && m.nan_fill == 1000.0f && m.mincov_gate == -inf);
    }
    // the driver: defaults, cset_vect of :56, refusals, stage seeds
    {
        DriverPrm p = driver_defaults();
        EXPECT(check_driver(buf, sizeof buf, p) == nullptr);
        const std::vector<double> cs = cset_vector(p.ransac_min_cset, p.ransac_max_cset, p.ransac_cset_cycles);
        EXPECT(cs.size() == 11 && cs[0] == 0.1 && cs[10] == 0.1 + (0.7 - 0.1) / 10 * 10.0);
        EXPECT(cset_vector(0.1, 0.7, 1).size() == 2 && cset_vector(0.1, 0.7, 65535).size() == 65536);
        for (int bad : {INT_MIN, 0, 65536, INT_MAX}) {
            DriverPrm q = p;
            q.ransac_cset_cycles = bad;
            EXPECT(check_driver(buf, sizeof buf, q) != nullptr);
        }
        for (int bad : {INT_MIN, -1, 0, 32768, INT_MAX}) {
            DriverPrm q = p;
            q.seeds = bad;
            EXPECT(check_driver(buf, sizeof buf, q) != nullptr);
        }
        DriverPrm q = p;
        q.gen_scl = nan;
        EXPECT(check_driver(buf, sizeof buf, q) != nullptr);
        q = p;
        q.rc_scl = 0.0;
        EXPECT(check_driver(buf, sizeof buf, q) != nullptr);
        q = p;
        q.srem_thr = inf;
        EXPECT(check_driver(buf, sizeof buf, q) != nullptr);
        EXPECT(stage_seed(5, 0) == 5 && stage_seed(5, 3) == 5 + (3ull << 32));
        EXPECT(stage_seed(~0ull, 1) == (1ull << 32) - 1); // 64-bit wrapping
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
