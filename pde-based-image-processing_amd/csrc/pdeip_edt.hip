// pdeip_edt.hip -- libpdeip.so: the exact Euclidean distance transform and what stands on it.
//
//   squared distance, nearest feature's index and distance of every pixel, ties to the lowest index   pdeip_edt(_dev)
//   [D, IDX] = bwdist(BW)                                                                             pdeip_bwdist(_dev)
//   the signed distance of the level set A >= 0, the interface half-way between the pixels           pdeip_signed_distance(_dev)
//   holes (NaN) of a sparse map filled with the nearest known pixel's bits                           pdeip_nearest_fill(_dev)
//   cross-checks, splat, nearest-source fill and blend as one resident chain                          pdeip_flow_interpolate_nearest(_dev)
//
// Kernels: csrc/pdeip_edt.hpp; the contract: include/pdeip.h.  No call has an ordering, so pdeip_set_mode does not apply.  Nothing is
// read back in the _dev forms and no launch depends on the data.
//
// Build (build.py): hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -c, one object per translation unit.
#include "pdeip_ctx.hpp"
#include "pdeip_edt.hpp"

#include <cmath>

using namespace pdeip;
using namespace pdeip::edt;

namespace {

constexpr int MAX_SIDE = 32767; // d2 <= 2 * 32766^2 fits an int32
constexpr int EDT_LAUNCHES = 2, SDF_LAUNCHES = 2 * EDT_LAUNCHES + 1, FILL_LAUNCHES = EDT_LAUNCHES + 1;

// Everything refused is refused here, before any HIP call.
int shape_args(const char *who, int nrows, int ncols, int frames)
{
    if (frames < 1) return set_err(PDEIP_ERR_ARG, "%s: frames must be >= 1 (got %d)", who, frames);
    if (nrows < 1 || ncols < 1) return set_err(PDEIP_ERR_ARG, "%s: the plane must be at least 1x1 (got %dx%d)", who, nrows, ncols);
    if (nrows > MAX_SIDE || ncols > MAX_SIDE)
        return set_err(PDEIP_ERR_UNSUPPORTED, "%s: a side above %d (got %dx%d): the squared distance must fit an int32", who, MAX_SIDE, nrows, ncols);
    if ((long long)nrows * ncols * frames > 0x7fffffffLL) return set_err(PDEIP_ERR_ARG, "%s: more than 2^31-1 elements", who);
    return PDEIP_OK;
}

int mode_arg(const char *who, int mode)
{
    if (mode < 0 || mode > 6 || (mode & 3) == 3)
        return set_err(PDEIP_ERR_ARG, "%s: unknown mode %d (PDEIP_EDT_POSITIVE, _NONNEG, _NOT_NAN and their _NOT twins)", who, mode);
    return PDEIP_OK;
}

int edt_args(const char *who, const void *A, int nrows, int ncols, int frames, int mode, const void *d2_out, const void *idx_out,
             const void *dist_out)
{
    NONNULL(who, A);
    if (d2_out == nullptr && idx_out == nullptr && dist_out == nullptr)
        return set_err(PDEIP_ERR_ARG, "%s: d2_out, idx_out and dist_out are all NULL", who);
    RC(mode_arg(who, mode));
    return shape_args(who, nrows, ncols, frames);
}

int bwdist_args(const char *who, const void *BW, int nrows, int ncols, int frames, const void *D_out, const void *idx_out)
{
    NONNULL(who, BW);
    if (D_out == nullptr && idx_out == nullptr) return set_err(PDEIP_ERR_ARG, "%s: D_out and idx_out are both NULL", who);
    return shape_args(who, nrows, ncols, frames);
}

int sdf_args(const char *who, const void *A, int nrows, int ncols, int frames, const void *out)
{
    NONNULL(who, A); NONNULL(who, out);
    return shape_args(who, nrows, ncols, frames);
}

int fill_args(const char *who, const void *D, int nrows, int ncols, int frames, const void *out, const void *filled_out, const void *dist_out)
{
    NONNULL(who, D); NONNULL(who, out);
    RC(shape_args(who, nrows, ncols, frames));
    if (filled_out != nullptr && (filled_out == D || filled_out == out)) return set_err(PDEIP_ERR_ARG, "%s: filled_out is D or out", who);
    if (dist_out != nullptr && (dist_out == D || dist_out == out || dist_out == filled_out))
        return set_err(PDEIP_ERR_ARG, "%s: dist_out is D, out or filled_out", who);
    return PDEIP_OK;
}

unsigned flat_blocks(size_t n)
{
    size_t blocks = (n + FLAT_BLOCK - 1) / FLAT_BLOCK;
    if (blocks > 256 * 16) blocks = 256 * 16; // grid-stride beyond 16 workgroups per compute unit
    return (unsigned)blocks;
}

// The transform's two launches on s.  G: nrows * ncols * frames ints of device memory.
int run_edt(hipStream_t s, const float *A, int nrows, int ncols, int frames, int mode, int max_dist, int *G, int *d2_out, int *idx_out,
            float *dist_out)
{
    const int row_blocks = (nrows + ROW_BLOCK - 1) / ROW_BLOCK;
    const size_t columns = (size_t)ncols * frames, units = (size_t)row_blocks * frames;
    const auto capped = [](size_t v) { return (unsigned)(v < MAX_UNITS ? v : MAX_UNITS); };
    hipLaunchKernelGGL(k_edt_cols, dim3(capped(columns)), dim3(COL_BLOCK), 0, s, A, G, nrows, columns, mode, max_dist);
    hipLaunchKernelGGL(k_edt_rows, dim3(capped(units), (unsigned)ncols), dim3(ROW_BLOCK), 0, s, G, nrows, ncols, row_blocks, units, max_dist,
                       d2_out, idx_out, dist_out);
    HIPCHK(hipGetLastError());
    return PDEIP_OK;
}

// Workspace (WS_EDT): `planes` planes of pad4(N) 4-byte words, the first one the column pass's offsets.
int edt_ws(size_t N, int planes, int **G, float **P1, float **P2)
{
    float *ws = nullptr;
    RC(ws_get(WS_EDT, (size_t)planes * pad4(N) * sizeof(float), &ws));
    *G = reinterpret_cast<int *>(ws);
    if (P1 != nullptr) *P1 = ws + pad4(N);
    if (P2 != nullptr) *P2 = ws + 2 * pad4(N);
    return PDEIP_OK;
}

float sdf_none(int max_dist) { return max_dist > 0 ? (float)((double)max_dist + 1.0) : INFINITY; }

// The interpolation chain's parameters with the defaults filled in, and its refusals (those of pdeip_flow_interpolate without the hole
// filling's parameters).
struct Resolved {
    double a, b;
    int use_costs;
};

int chain_args(const char *who, const void *I0, const void *I1, int channels, const void *Uf, const void *Vf, const void *Ub, const void *Vb,
               int nrows, int ncols, double t, const pdeip_interp_params *prm, const void *It_out, const void *Ut_out, const void *Vt_out,
               const void *source_out, Resolved *p)
{
    NONNULL(who, I0); NONNULL(who, I1); NONNULL(who, Uf); NONNULL(who, Vf); NONNULL(who, It_out);
    if (channels < 1) return set_err(PDEIP_ERR_ARG, "%s: channels must be >= 1 (got %d)", who, channels);
    if ((Ub != nullptr) != (Vb != nullptr)) return set_err(PDEIP_ERR_ARG, "%s: Ub and Vb must both be given or both be NULL", who);
    if (!(t > 0.0 && t < 1.0)) return set_err(PDEIP_ERR_ARG, "%s: t must lie strictly between 0 and 1 (got %g)", who, t);
    if (nrows < 3 || ncols < 3) return set_err(PDEIP_ERR_ARG, "%s: the field must be at least 3x3 (got %dx%d)", who, nrows, ncols);
    RC(shape_args(who, nrows, ncols, 2));
    *p = Resolved{0.01, 0.5, 1};
    if (prm != nullptr) {
        if (prm->fill != nullptr) return set_err(PDEIP_ERR_ARG, "%s: prm->fill must be NULL (the nearest-source fill has no TV parameters)", who);
        *p = Resolved{prm->a, prm->b, prm->use_costs != 0};
    }
    if (!(p->a >= 0.0) || !(p->b >= 0.0)) return set_err(PDEIP_ERR_ARG, "%s: a and b must be >= 0 and not NaN (got %g, %g)", who, p->a, p->b);
    const void *outs[4] = {It_out, Ut_out, Vt_out, source_out};
    const void *ins[6] = {I0, I1, Uf, Vf, Ub, Vb};
    for (const void *o : outs)
        for (const void *in : ins)
            if (o != nullptr && o == in) return set_err(PDEIP_ERR_ARG, "%s: an output pointer equals an input pointer", who);
    return PDEIP_OK;
}

// The chain's scratch, in floats: the two masks, the splatted flow [nrows x ncols x 2] and the filled one.
size_t chain_scratch(size_t n) { return 2 * pad4(n) + 2 * pad4(2 * n); }

// Cross-checks, splat, nearest-source fill, blend on s.  scratch: chain_scratch(n) floats; G, IDX: n ints each.
int run_chain(hipStream_t s, const float *I0, const float *I1, int channels, const float *Uf, const float *Vf, const float *Ub, const float *Vb,
              int nrows, int ncols, double t, const Resolved &p, int max_dist, float *scratch, int *G, int *IDX, float *It_out, float *Ut_out,
              float *Vt_out, float *source_out)
{
    const size_t n = (size_t)nrows * ncols;
    float *M0 = scratch, *M1 = M0 + pad4(n), *S = M1 + pad4(n), *F = S + pad4(2 * n);
    int launches = 0;
    const bool masks = Ub != nullptr;
    if (masks) {
        RC(pdeip_flow_crosscheck_dev(s, Uf, Vf, Ub, Vb, nrows, ncols, p.a, p.b, M0, nullptr, nullptr));
        launches += tls.last_launches;
        RC(pdeip_flow_crosscheck_dev(s, Ub, Vb, Uf, Vf, nrows, ncols, p.a, p.b, M1, nullptr, nullptr));
        launches += tls.last_launches;
    }
    const bool costs = p.use_costs != 0;
    RC(pdeip_flow_splat_dev(s, Uf, Vf, costs ? I0 : nullptr, costs ? I1 : nullptr, channels, nrows, ncols, t, S, S + n, nullptr));
    launches += tls.last_launches;
    // the splat gives both planes the same holes: one transform of Ut's serves both
    RC(run_edt(s, S, nrows, ncols, 1, PDEIP_EDT_NOT_NAN, max_dist, G, nullptr, IDX, nullptr));
    launches += EDT_LAUNCHES;
    hipLaunchKernelGGL(k_nearest_gather, dim3(flat_blocks(2 * n)), dim3(FLAT_BLOCK), 0, s, reinterpret_cast<const unsigned *>(S), IDX, n,
                       (size_t)0, 2 * n, 1, reinterpret_cast<unsigned *>(F), (float *)nullptr);
    HIPCHK(hipGetLastError());
    launches++;
    RC(pdeip_interp_blend_dev(s, I0, I1, channels, F, F + n, masks ? M0 : nullptr, masks ? M1 : nullptr, nrows, ncols, t, It_out, source_out));
    launches += tls.last_launches;
    if (Ut_out != nullptr) {
        RC(copy_d2d(s, Ut_out, F, n));
        launches++;
    }
    if (Vt_out != nullptr) {
        RC(copy_d2d(s, Vt_out, F + n, n));
        launches++;
    }
    const int expected = (masks ? 2 : 0) + 3 + EDT_LAUNCHES + 1 + 1 + (Ut_out != nullptr) + (Vt_out != nullptr);
    if (launches != expected)
        return set_err(PDEIP_ERR_DEVICE, "pdeip_flow_interpolate_nearest: %d launches where %d are stated", launches, expected);
    tls.last_launches = launches;
    return PDEIP_OK;
}

} // namespace

// Launches: 2 (columns, rows), whatever the data.  Workspace (WS_EDT): one int per element.
extern "C" int pdeip_edt_dev(void *stream, const float *A, int nrows, int ncols, int frames, int mode, int max_dist, int *d2_out, int *idx_out,
                             float *dist_out)
{
    const char *who = "pdeip_edt_dev";
    RC(edt_args(who, A, nrows, ncols, frames, mode, d2_out, idx_out, dist_out));
    int *G = nullptr;
    RC(edt_ws((size_t)nrows * ncols * frames, 1, &G, nullptr, nullptr));
    RC(run_edt(static_cast<hipStream_t>(stream), A, nrows, ncols, frames, mode, max_dist, G, d2_out, idx_out, dist_out));
    tls.last_launches = EDT_LAUNCHES;
    return PDEIP_OK;
}

extern "C" int pdeip_edt(const float *A, int nrows, int ncols, int frames, int mode, int max_dist, int *d2_out, int *idx_out, float *dist_out)
{
    const char *who = "pdeip_edt";
    RC(edt_args(who, A, nrows, ncols, frames, mode, d2_out, idx_out, dist_out));
    RC(use_device());
    const size_t N = (size_t)nrows * ncols * frames, pN = pad4(N);
    // arena: A, then d2, idx, dist
    float *ar = nullptr;
    RC(ws_get(WS_ARENA, 4 * pN * sizeof(float), &ar));
    int *dd2 = d2_out ? reinterpret_cast<int *>(ar + pN) : nullptr, *didx = idx_out ? reinterpret_cast<int *>(ar + 2 * pN) : nullptr;
    float *ddist = dist_out ? ar + 3 * pN : nullptr;
    HIPCHK(hipMemcpy(ar, A, N * sizeof(float), hipMemcpyHostToDevice));
    RC(pdeip_edt_dev(nullptr, ar, nrows, ncols, frames, mode, max_dist, dd2, didx, ddist));
    if (d2_out) HIPCHK(hipMemcpy(d2_out, dd2, N * sizeof(int), hipMemcpyDeviceToHost));
    if (idx_out) HIPCHK(hipMemcpy(idx_out, didx, N * sizeof(int), hipMemcpyDeviceToHost));
    if (dist_out) HIPCHK(hipMemcpy(dist_out, ddist, N * sizeof(float), hipMemcpyDeviceToHost));
    return PDEIP_OK;
}

// Launches: 2, the transform's.
extern "C" int pdeip_bwdist_dev(void *stream, const float *BW, int nrows, int ncols, int frames, float *D_out, int *idx_out)
{
    const char *who = "pdeip_bwdist_dev";
    RC(bwdist_args(who, BW, nrows, ncols, frames, D_out, idx_out));
    int *G = nullptr;
    RC(edt_ws((size_t)nrows * ncols * frames, 1, &G, nullptr, nullptr));
    RC(run_edt(static_cast<hipStream_t>(stream), BW, nrows, ncols, frames, PDEIP_EDT_POSITIVE, 0, G, nullptr, idx_out, D_out));
    tls.last_launches = EDT_LAUNCHES;
    return PDEIP_OK;
}

extern "C" int pdeip_bwdist(const float *BW, int nrows, int ncols, int frames, float *D_out, int *idx_out)
{
    const char *who = "pdeip_bwdist";
    RC(bwdist_args(who, BW, nrows, ncols, frames, D_out, idx_out));
    return pdeip_edt(BW, nrows, ncols, frames, PDEIP_EDT_POSITIVE, 0, nullptr, idx_out, D_out);
}

// Launches: 5 (the transform of the outside, the transform of the inside, the combination).  Workspace (WS_EDT): three planes.
extern "C" int pdeip_signed_distance_dev(void *stream, const float *A, int nrows, int ncols, int frames, int max_dist, float *out)
{
    const char *who = "pdeip_signed_distance_dev";
    RC(sdf_args(who, A, nrows, ncols, frames, out));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t N = (size_t)nrows * ncols * frames;
    int *G = nullptr;
    float *to_out = nullptr, *to_in = nullptr;
    RC(edt_ws(N, 3, &G, &to_out, &to_in));
    RC(run_edt(s, A, nrows, ncols, frames, PDEIP_EDT_NONNEG_NOT, max_dist, G, nullptr, nullptr, to_out));
    RC(run_edt(s, A, nrows, ncols, frames, PDEIP_EDT_NONNEG, max_dist, G, nullptr, nullptr, to_in));
    hipLaunchKernelGGL(k_sdf_combine, dim3(flat_blocks(N)), dim3(FLAT_BLOCK), 0, s, A, to_out, to_in, sdf_none(max_dist), N, out);
    HIPCHK(hipGetLastError());
    tls.last_launches = SDF_LAUNCHES;
    return PDEIP_OK;
}

extern "C" int pdeip_signed_distance(const float *A, int nrows, int ncols, int frames, int max_dist, float *out)
{
    const char *who = "pdeip_signed_distance";
    RC(sdf_args(who, A, nrows, ncols, frames, out));
    RC(use_device());
    const size_t N = (size_t)nrows * ncols * frames, pN = pad4(N);
    float *ar = nullptr; // arena: A, out
    RC(ws_get(WS_ARENA, 2 * pN * sizeof(float), &ar));
    HIPCHK(hipMemcpy(ar, A, N * sizeof(float), hipMemcpyHostToDevice));
    RC(pdeip_signed_distance_dev(nullptr, ar, nrows, ncols, frames, max_dist, ar + pN));
    HIPCHK(hipMemcpy(out, ar + pN, N * sizeof(float), hipMemcpyDeviceToHost));
    return PDEIP_OK;
}

// Launches: 3 (the transform of the known pixels, the gather).  Workspace (WS_EDT): two planes.
extern "C" int pdeip_nearest_fill_dev(void *stream, const float *D, int nrows, int ncols, int frames, int max_dist, float *out, float *filled_out,
                                      float *dist_out)
{
    const char *who = "pdeip_nearest_fill_dev";
    RC(fill_args(who, D, nrows, ncols, frames, out, filled_out, dist_out));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t n = (size_t)nrows * ncols, N = n * frames;
    int *G = nullptr;
    float *idx = nullptr;
    RC(edt_ws(N, 2, &G, &idx, nullptr));
    int *IDX = reinterpret_cast<int *>(idx);
    RC(run_edt(s, D, nrows, ncols, frames, PDEIP_EDT_NOT_NAN, max_dist, G, nullptr, IDX, dist_out));
    hipLaunchKernelGGL(k_nearest_gather, dim3(flat_blocks(N)), dim3(FLAT_BLOCK), 0, s, reinterpret_cast<const unsigned *>(D), IDX, n, n, N, 0,
                       reinterpret_cast<unsigned *>(out), filled_out);
    HIPCHK(hipGetLastError());
    tls.last_launches = FILL_LAUNCHES;
    return PDEIP_OK;
}

extern "C" int pdeip_nearest_fill(const float *D, int nrows, int ncols, int frames, int max_dist, float *out, float *filled_out, float *dist_out)
{
    const char *who = "pdeip_nearest_fill";
    RC(fill_args(who, D, nrows, ncols, frames, out, filled_out, dist_out));
    RC(use_device());
    const size_t N = (size_t)nrows * ncols * frames, pN = pad4(N);
    float *ar = nullptr; // arena: D (filled in place), filled, dist
    RC(ws_get(WS_ARENA, 3 * pN * sizeof(float), &ar));
    float *dfilled = filled_out ? ar + pN : nullptr, *ddist = dist_out ? ar + 2 * pN : nullptr;
    HIPCHK(hipMemcpy(ar, D, N * sizeof(float), hipMemcpyHostToDevice));
    RC(pdeip_nearest_fill_dev(nullptr, ar, nrows, ncols, frames, max_dist, ar, dfilled, ddist));
    HIPCHK(hipMemcpy(out, ar, N * sizeof(float), hipMemcpyDeviceToHost));
    if (filled_out) HIPCHK(hipMemcpy(filled_out, dfilled, N * sizeof(float), hipMemcpyDeviceToHost));
    if (dist_out) HIPCHK(hipMemcpy(dist_out, ddist, N * sizeof(float), hipMemcpyDeviceToHost));
    return PDEIP_OK;
}

// Launches: [2 with Ub, Vb] + 3 (splat) + 2 (transform) + 1 (gather of both planes) + 1 (blend) + one per Ut_out / Vt_out given.
// Scratch: chain_scratch() floats (WS_ARENA), two planes (WS_EDT).
extern "C" int pdeip_flow_interpolate_nearest_dev(void *stream, const float *I0, const float *I1, int channels, const float *Uf, const float *Vf,
                                                  const float *Ub, const float *Vb, int nrows, int ncols, double t,
                                                  const pdeip_interp_params *prm, int max_dist, float *It_out, float *Ut_out, float *Vt_out,
                                                  float *source_out)
{
    const char *who = "pdeip_flow_interpolate_nearest_dev";
    Resolved p;
    RC(chain_args(who, I0, I1, channels, Uf, Vf, Ub, Vb, nrows, ncols, t, prm, It_out, Ut_out, Vt_out, source_out, &p));
    const size_t n = (size_t)nrows * ncols;
    float *scratch = nullptr, *idx = nullptr;
    int *G = nullptr;
    RC(ws_get(WS_ARENA, chain_scratch(n) * sizeof(float), &scratch));
    RC(edt_ws(n, 2, &G, &idx, nullptr));
    return run_chain(static_cast<hipStream_t>(stream), I0, I1, channels, Uf, Vf, Ub, Vb, nrows, ncols, t, p, max_dist, scratch, G,
                     reinterpret_cast<int *>(idx), It_out, Ut_out, Vt_out, source_out);
}

extern "C" int pdeip_flow_interpolate_nearest(const float *I0, const float *I1, int channels, const float *Uf, const float *Vf, const float *Ub,
                                              const float *Vb, int nrows, int ncols, double t, const pdeip_interp_params *prm, int max_dist,
                                              float *It_out, float *Ut_out, float *Vt_out, float *source_out)
{
    const char *who = "pdeip_flow_interpolate_nearest";
    Resolved p;
    RC(chain_args(who, I0, I1, channels, Uf, Vf, Ub, Vb, nrows, ncols, t, prm, It_out, Ut_out, Vt_out, source_out, &p));
    RC(use_device());
    const size_t n = (size_t)nrows * ncols, pn = pad4(n), pc = pad4(n * channels);
    // arena: the chain's scratch, then I0, I1, It, then Uf, Vf, Ub, Vb, Ut, Vt, source
    float *ar = nullptr, *idx = nullptr;
    int *G = nullptr;
    RC(ws_get(WS_ARENA, (chain_scratch(n) + 3 * pc + 7 * pn) * sizeof(float), &ar));
    RC(edt_ws(n, 2, &G, &idx, nullptr));
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
    RC(run_chain(nullptr, dI0, dI1, channels, dUf, dVf, dUb, dVb, nrows, ncols, t, p, max_dist, ar, G, reinterpret_cast<int *>(idx), dIt, dUt,
                 dVt, dsrc));
    HIPCHK(hipMemcpy(It_out, dIt, n * channels * sizeof(float), hipMemcpyDeviceToHost));
    if (Ut_out) HIPCHK(hipMemcpy(Ut_out, dUt, n * sizeof(float), hipMemcpyDeviceToHost));
    if (Vt_out) HIPCHK(hipMemcpy(Vt_out, dVt, n * sizeof(float), hipMemcpyDeviceToHost));
    if (source_out) HIPCHK(hipMemcpy(source_out, dsrc, n * sizeof(float), hipMemcpyDeviceToHost));
    return PDEIP_OK;
}
