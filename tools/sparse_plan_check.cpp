// sparse_plan_check.cpp -- the host-side decisions of the sparse driver's calls (csrc/pdeip_sparse_plan.hpp: the argument checks of
// pdeip_nanmedfilt2 and pdeip_sparse_pyramid, the scale sizes, the layout of the pyramid and of the builder's temporaries, the
// constants of the sparse stages) exercised on their own, for the host sanitizers:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/sparse_plan_check.cpp -o sparse_plan_check && ./sparse_plan_check
//
// No HIP and no GPU: nothing here is loaded into another process.  Exit status 0 and "ok" on success.
#include "../pde-based-image-processing_amd/csrc/pdeip_sparse_plan.hpp"

#include <climits>
#include <cstring>

using namespace pdeip;

static int failures = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("%s:%d: %s is false\n", __FILE__, __LINE__, #cond); \
            failures++;                                                    \
        }                                                                  \
    } while (0)

static const float PLANE[4] = {0, 0, 0, 0};
static float OUT[4];

static bool filter_refused(const char *word, const void *A, const void *out, int nr, int nc, int nf, bool want_unsupported = false)
{
    char buf[160];
    bool unsupported = !want_unsupported;
    const char *m = sparse::check_filter(buf, sizeof buf, A, out, nr, nc, nf, &unsupported);
    return m != nullptr && std::strstr(m, word) != nullptr && unsupported == want_unsupported;
}

static bool pyramid_refused(const char *word, int nr, int nc, double f, double ps, int cap)
{
    char buf[160];
    const char *m = sparse::check_pyramid(buf, sizeof buf, nr, nc, f, ps, cap);
    return m != nullptr && std::strstr(m, word) != nullptr;
}

int main()
{
    char buf[160];
    bool u = true;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();

    // pdeip_nanmedfilt2: accepted down to 1x1 and up to a plane of INT_MAX pixels
    EXPECT(sparse::check_filter(buf, sizeof buf, PLANE, OUT, 1, 1, 1, &u) == nullptr && !u);
    EXPECT(sparse::check_filter(buf, sizeof buf, PLANE, OUT, 2160, 3840, 3, &u) == nullptr);
    EXPECT(sparse::check_filter(buf, sizeof buf, PLANE, OUT, INT_MAX, 1, 1, &u) == nullptr);
    EXPECT(sparse::check_filter(buf, sizeof buf, PLANE, OUT, 46340, 46340, 65535, &u) == nullptr);
    EXPECT(filter_refused("'A' is NULL", nullptr, OUT, 4, 4, 1));
    EXPECT(filter_refused("'out' is NULL", PLANE, nullptr, 4, 4, 1));
    for (int bad : {INT_MIN, -1, 0}) {
        EXPECT(filter_refused("1x1", PLANE, OUT, bad, 4, 1));
        EXPECT(filter_refused("1x1", PLANE, OUT, 4, bad, 1));
        EXPECT(filter_refused("frames", PLANE, OUT, 4, 4, bad));
    }
    EXPECT(filter_refused("INT_MAX", PLANE, OUT, INT_MAX, 2, 1));
    EXPECT(filter_refused("INT_MAX", PLANE, OUT, INT_MAX, INT_MAX, INT_MAX));
    EXPECT(filter_refused("INT_MAX", PLANE, OUT, 46341, 46341, 1));
    EXPECT(filter_refused("alias", PLANE, PLANE, 2, 2, 1));
    EXPECT(filter_refused("columns or frames", PLANE, OUT, 4, 65536, 1, true));
    EXPECT(filter_refused("columns or frames", PLANE, OUT, 4, 4, 65536, true));

    // pdeip_sparse_pyramid
    EXPECT(sparse::check_pyramid(buf, sizeof buf, 3, 3, 0.75, 0.55, 1) == nullptr);
    EXPECT(sparse::check_pyramid(buf, sizeof buf, 32768, 65535, 0.75, 0.55, 64) == nullptr);
    EXPECT(pyramid_refused("3x3", 2, 8, 0.75, 0.55, 8));
    EXPECT(pyramid_refused("3x3", 8, INT_MIN, 0.75, 0.55, 8));
    EXPECT(pyramid_refused("INT_MAX", INT_MAX, INT_MAX, 0.75, 0.55, 8));
    for (double f : {nan, 0.0, 1.0, -0.5, inf}) EXPECT(pyramid_refused("scl_factor", 8, 8, f, 0.55, 8));
    for (double p : {nan, 0.0, -0.5, inf}) EXPECT(pyramid_refused("pyr_scl", 8, 8, 0.75, p, 8));
    for (int cap : {INT_MIN, -1, 0}) EXPECT(pyramid_refused("scales_cap", 8, 8, 0.75, 0.55, cap));

    // the sizes the driver meets, and the layout of every pyramid up to planes of INT_MAX pixels
    {
        const std::vector<seeds::Size> t = seeds::scale_sizes(60, 80, 0.75, 0.55);
        EXPECT(t.size() == 3 && t[1].r == 45 && t[1].c == 60 && t[2].r == 34 && t[2].c == 45);
        const sparse::Layout L = sparse::layout(t);
        EXPECT(L.launches == 7 && L.scale.size() == 3 && L.scale[0] == 0 && L.scale[1] == 4800 && L.scale[2] == 7500);
        EXPECT(L.t1 == 7500 + 1532 && L.t2 == L.t1 + 4800 && L.total == L.t2 + 2700);
        EXPECT(sparse::packed_floats(t) == 4800 + 2700 + 1530);
        const std::vector<seeds::Size> g = seeds::scale_sizes(288, 384, 0.75, 0.55);
        EXPECT(g.size() == 3 && g[1].r == 216 && g[1].c == 288 && g[2].r == 162 && g[2].c == 216);
        const std::vector<seeds::Size> one = seeds::scale_sizes(3, 3, 0.75, 0.55);
        const sparse::Layout L1 = sparse::layout(one);
        EXPECT(one.size() == 1 && L1.launches == 1 && L1.total == 12 && L1.t1 == 12 && L1.t2 == 12); // no temporaries without a second scale
    }
    const int shapes[][2] = {{3, 3}, {3, 5}, {37, 53}, {60, 80}, {288, 384}, {2160, 3840}, {46340, 46340}, {32768, 65535}, {INT_MAX / 3, 3}, {3, 65535}};
    for (const auto &sh : shapes)
        for (double f : {1e-9, 0.3, 0.5, 0.75, 0.99, 0.999999999})
            for (double ps : {1e-9, 0.2, 0.55, 1.0, 7.0}) {
                const int nr = sh[0], nc = sh[1];
                EXPECT(sparse::check_pyramid(buf, sizeof buf, nr, nc, f, ps, 1) == nullptr);
                const std::vector<seeds::Size> sz = seeds::scale_sizes(nr, nc, f, ps);
                const sparse::Layout L = sparse::layout(sz);
                const size_t K = sz.size();
                EXPECT(K >= 1 && L.scale.size() == K && L.launches == 3 * (int)K - 2);
                size_t packed = 0;
                for (size_t k = 0; k < K; k++) {
                    const size_t n = sparse::pixels(sz[k]);
                    EXPECT(n == (size_t)sz[k].r * (size_t)sz[k].c && n <= (size_t)INT_MAX);
                    EXPECT(L.scale[k] % 4 == 0);
                    const size_t end = k + 1 < K ? L.scale[k + 1] : L.t1;
                    EXPECT(L.scale[k] + n <= end && end - L.scale[k] < n + 4); // the planes do not overlap and are packed to 4 floats
                    packed += n;
                }
                EXPECT(sparse::packed_floats(sz) == packed);
                EXPECT(L.t1 % 4 == 0 && L.t2 % 4 == 0 && L.total % 4 == 0 && L.t1 <= L.t2 && L.t2 <= L.total);
                if (K > 1) {
                    EXPECT(L.t2 - L.t1 >= sparse::pixels(sz[0]));    // t1 holds nanmed(P_k) of the largest scale
                    EXPECT(L.total - L.t2 >= sparse::pixels(sz[1])); // t2 holds its resize: no scale after the second is larger
                    for (size_t k = 1; k < K; k++) EXPECT(sparse::pixels(sz[k]) <= sparse::pixels(sz[1]) && sparse::pixels(sz[k - 1]) <= sparse::pixels(sz[0]));
                } else {
                    EXPECT(L.t1 == L.t2 && L.t2 == L.total);
                }
            }

    // the constants: what a NaN member or a NULL struct resolves to in the two forms
    {
        const seeds::Prm s = sparse::resolve(sparse::seeds_defaults(), nullptr, nullptr, nullptr);
        EXPECT(s.dist_cap == 100.0 && s.nan_fill == 1000.0f && s.mincov_gate == 0.5);
        const seeds::Prm d = sparse::resolve(sparse::dense_seeds_defaults(), nullptr, nullptr, nullptr);
        EXPECT(d.dist_cap == inf && d.mincov_gate == -inf && std::isnan(d.nan_fill));
        const double cap = 50.0, gate = 0.25;
        const seeds::Prm m = sparse::resolve(sparse::seeds_defaults(), &cap, &nan, &gate);
        EXPECT(m.dist_cap == 50.0 && m.nan_fill == 1000.0f && m.mincov_gate == 0.25);
        const seeds::Prm e = sparse::resolve(sparse::dense_seeds_defaults(), &cap, &nan, &nan); // the dense form is seeds::resolve
        const seeds::Prm e2 = seeds::resolve(&cap, &nan, &nan);
        EXPECT(e.dist_cap == e2.dist_cap && e.mincov_gate == e2.mincov_gate && std::isnan(e.nan_fill) && std::isnan(e2.nan_fill));
        EXPECT(sparse::GAMMA0 == 0.005 && seeds::GAMMA0 == 0.01);
        const seeds::DriverPrm p = sparse::driver_defaults();
        EXPECT(p.srem_thr == 0.002 && p.scl_factor == 0.75 && p.gen_scl == 0.55 && p.rc_scl == 0.55 && p.ransac_min_cset == 0.1 &&
               p.ransac_max_cset == 0.7 && p.polyorder == 2 && p.seeds == 15 && p.ransac_cset_cycles == 10);
        EXPECT(seeds::check_driver(buf, sizeof buf, p) == nullptr);
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
