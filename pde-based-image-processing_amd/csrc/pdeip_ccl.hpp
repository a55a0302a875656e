// pdeip_ccl.hpp -- kernels of connected-component labelling: bwlabel(A > 0) with MATLAB's numbering, the areas of regionprops and
// the largest component, as generateSeeds() uses them (matlab/segmentation/DispSegmentation.m:282-298).  The contract is in
// include/pdeip.h; tests/ccl_ref.py restates it.
//
// A component's representative is its smallest column-major linear index, so MATLAB's order of the components is the order of
// the roots, and a label is 1 + the number of roots before it: a prefix sum over root flags.  The forest is an int plane T with
// T[p] <= p (-1: background); two trees are merged by an integer atomicMin on the larger root, whose outcome does not depend on
// who comes first.  No floating-point atomics anywhere.
//
//   the tiled form (any size), a launch count that does not depend on the mask:
//   k_ccl_local    one workgroup per TILE_I x TILE_J tile, entirely in LDS: a wave runs down a tile column, __ballot gives every
//                  pixel the start of its vertical run, runs of neighbouring columns are merged with LDS atomicMin; T receives
//                  the tile root as a global index.  No global atomic.
//   k_ccl_seam     only the pixels on inner tile borders: global atomicMin unions with the neighbouring tile's border (the three
//                  west neighbours across a column seam, north and the two upper diagonals across a row seam).
//   k_ccl_flatten  every pixel reads its root (the walk halves the path as it goes); counts the roots of each LIN_PIX pixels;
//                  clears the area table.
//   k_ccl_scan     exclusive prefix sum of those counts by one workgroup (the two-level integer scan of k_mask_count /
//                  k_mask_scan, pdeip_ransac.hpp, mirrored); the total is num.
//   k_ccl_rank     roots write their label; k_ccl_relabel: everyone else copies its root's, and the areas are counted per (block,
//                  label) in an LDS table, then one global integer add per pair.
//   k_ccl_argmax / k_ccl_select   the largest area (lowest label on a tie) and the two-valued plane.
//
//   the small form (npix <= SMALL_MAX_PIX: the coarse pyramid scales the drivers call this on):
//   k_ccl_small    one workgroup, the forest and the counters in LDS, all of the above in one launch and no global atomic.
#pragma once
#include "pdeip_ctx.hpp"
#include "pdeip_ccl_plan.hpp"

namespace pdeip {
namespace ccl {

// Offset (0..lane) of the first pixel of the vertical run that `lane` belongs to, from the wave's foreground ballot.
__device__ inline int run_start(unsigned long long bal, int lane)
{
    const unsigned long long below = ~bal & ((1ull << lane) - 1ull);
    return below ? 64 - __clzll((long long)below) : 0;
}

// Which of the three pixels west of p (column j-1, rows i-1, i, i+1) p has to be merged with so that every adjacency between the
// two columns is merged by somebody: fg(di, dj) tells whether pixel (i+di, j+dj) is foreground (false outside the domain), un(di)
// merges p with (i+di, j-1).  W is skipped where N and NW are both set (N merges with NW, and N-p, NW-W are vertical runs); a
// diagonal only counts where W is background, and is skipped where the pixel above / below p sees it as its own W.
template <class Fg, class Un>
__device__ inline void west_rules(bool conn8, Fg fg, Un un)
{
    if (fg(0, -1)) {
        if (!(fg(-1, 0) && fg(-1, -1))) un(0);
    } else if (conn8) {
        if (fg(-1, -1) && !fg(-1, 0)) un(-1);
        if (fg(1, -1) && !fg(1, 0)) un(1);
    }
}

// ---- the forest in LDS ---------------------------------------------------------------------------------------------------------
__device__ inline int lds_find(volatile int *L, int a)
{
    int p = L[a];
    while (p != a) {
        a = p;
        p = L[a];
    }
    return a;
}

// Merges the trees of a and b: the larger root is pointed at the smaller one.  When the atomicMin finds that `a` was no root any
// more (old != a), the merge goes on from its old parent, so no link is lost whatever the interleaving.
__device__ inline void lds_union(int *L, int a, int b)
{
    a = lds_find(L, a);
    b = lds_find(L, b);
    while (a != b) {
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(&L[a], b);
        if (old == a) break;
        a = old;
    }
}

// ---- the forest in global memory -----------------------------------------------------------------------------------------------
__device__ inline int g_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Root of a; every node passed is pointed at its grandparent (an atomicMin: entries only ever decrease).
__device__ inline int g_find(int *T, int a)
{
    int p = g_load(T + a);
    while (p != a) {
        const int gp = g_load(T + p);
        if (gp != p) atomicMin(T + a, gp);
        a = p;
        p = gp;
    }
    return a;
}

__device__ inline void g_union(int *T, int a, int b)
{
    a = g_find(T, a);
    b = g_find(T, b);
    while (a != b) {
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(T + a, b);
        if (old == a) break;
        a = old;
    }
}

// ---- the tiled form ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TILE_THREADS) k_ccl_local(const float *__restrict__ A, int nrows, int ncols, int tiles_i, int conn8,
                                                           int *__restrict__ T)
{
    __shared__ int S[TILE_I * TILE_J]; // local index = 64*(tile column) + (tile row): the order of the global indices
    volatile int *vS = S;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ti = (int)(blockIdx.x % (unsigned)tiles_i), tj = (int)(blockIdx.x / (unsigned)tiles_i);
    const int i0 = ti * TILE_I, j0 = tj * TILE_J, i = i0 + lane;
    constexpr int COLS_PER_WAVE = TILE_J / (TILE_THREADS / 64);
#pragma unroll
    for (int c = 0; c < COLS_PER_WAVE; c++) {
        const int lj = wave + (TILE_THREADS / 64) * c, j = j0 + lj;
        const bool fg = i < nrows && j < ncols && A[(size_t)j * nrows + i] > 0.0f; // a NaN, both zeros and negatives are background
        const unsigned long long bal = __ballot(fg);
        S[lj * TILE_I + lane] = fg ? lj * TILE_I + run_start(bal, lane) : -1;
    }
    __syncthreads();
    for (int c = 0; c < COLS_PER_WAVE; c++) {
        const int lj = wave + (TILE_THREADS / 64) * c, idx = lj * TILE_I + lane;
        if (lj == 0 || vS[idx] < 0) continue;
        west_rules(conn8 != 0,
                   [&](int di, int dj) { const int li = lane + di; return li >= 0 && li < TILE_I && vS[(lj + dj) * TILE_I + li] >= 0; },
                   [&](int di) { lds_union(S, idx, (lj - 1) * TILE_I + lane + di); });
    }
    __syncthreads();
    for (int c = 0; c < COLS_PER_WAVE; c++) {
        const int lj = wave + (TILE_THREADS / 64) * c, j = j0 + lj;
        if (i >= nrows || j >= ncols) continue;
        const int v = vS[lj * TILE_I + lane];
        int root = -1;
        if (v >= 0) {
            const int r = lds_find(vS, v);
            root = (j0 + (r >> 6)) * nrows + i0 + (r & 63);
        }
        T[(size_t)j * nrows + i] = root;
    }
}

// items = nv + nh: the nv pixels of the columns j = TILE_J, 2 TILE_J, ... first, then the pixels of the rows i = TILE_I, 2 TILE_I, ...
__global__ void __launch_bounds__(LIN_THREADS) k_ccl_seam(int *T, int nrows, int ncols, int conn8, int nv, int items)
{
    const long long tl = (long long)blockIdx.x * LIN_THREADS + threadIdx.x;
    if (tl >= items) return;
    const int t = (int)tl;
    if (t < nv) {
        const int s = t / nrows, i = t - s * nrows, j = (s + 1) * TILE_J, p = j * nrows + i;
        if (T[p] < 0) return;
        west_rules(conn8 != 0,
                   [&](int di, int dj) { const int ii = i + di; return ii >= 0 && ii < nrows && T[p + dj * nrows + di] >= 0; },
                   [&](int di) { g_union(T, p, p - nrows + di); });
    } else {
        const int u = t - nv, s = u / ncols, j = u - s * ncols, i = (s + 1) * TILE_I, p = j * nrows + i;
        if (T[p] < 0) return;
        if (T[p - 1] >= 0) {
            g_union(T, p, p - 1);
        } else if (conn8) {
            if (j > 0 && T[p - 1 - nrows] >= 0) g_union(T, p, p - 1 - nrows);
            if (j < ncols - 1 && T[p - 1 + nrows] >= 0) g_union(T, p, p - 1 + nrows);
        }
    }
}

__device__ inline int block_total16(const int *s_w)
{
    int tot = 0;
#pragma unroll
    for (int w = 0; w < 16; w++) tot += s_w[w];
    return tot;
}

// T[p] = the root of p for every foreground pixel; blk_cnt[b] = the number of roots among pixels [b*LIN_PIX, (b+1)*LIN_PIX).
// Also clears areas[0..areas_cap) for k_ccl_relabel's adds (areas NULL: nothing to clear).
__global__ void __launch_bounds__(LIN_THREADS) k_ccl_flatten(int *T, int npix, int *__restrict__ blk_cnt, int *__restrict__ areas, int areas_cap)
{
    static_assert(LIN_PER_THREAD * (LIN_THREADS / 64) == 16, "block_total16");
    __shared__ int s_w[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long base = (long long)blockIdx.x * LIN_PIX;
    if (areas)
        for (long long k = (long long)blockIdx.x * LIN_THREADS + tid; k < areas_cap; k += (long long)gridDim.x * LIN_THREADS) areas[k] = 0;
#pragma unroll
    for (int k = 0; k < LIN_PER_THREAD; k++) {
        const long long pl = base + k * LIN_THREADS + tid;
        bool root = false;
        if (pl < npix) {
            const int p = (int)pl, q = g_load(T + p);
            if (q >= 0) {
                const int r = g_find(T, q);
                if (r != q) __hip_atomic_store(T + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                root = r == p;
            }
        }
        const int c = __popcll(__ballot(root));
        if (lane == 0) s_w[k * (LIN_THREADS / 64) + wave] = c;
    }
    __syncthreads();
    if (tid == 0) blk_cnt[blockIdx.x] = block_total16(s_w);
}

// Exclusive prefix sum of blk[0..nblk) in place by one workgroup; the total goes to total_a[0] and total_b[0] (NULL ok).
__global__ void __launch_bounds__(SCAN_THREADS) k_ccl_scan(int *__restrict__ blk, int nblk, int *__restrict__ total_a, int *__restrict__ total_b)
{
    __shared__ int s[SCAN_THREADS];
    __shared__ int s_carry;
    const int tid = threadIdx.x;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (int base = 0; base < nblk; base += SCAN_THREADS) {
        const int k = base + tid;
        const int v = k < nblk ? blk[k] : 0;
        s[tid] = v;
        __syncthreads();
        for (int d = 1; d < SCAN_THREADS; d <<= 1) {
            const int add = tid >= d ? s[tid - d] : 0;
            __syncthreads();
            s[tid] += add;
            __syncthreads();
        }
        const int carry = s_carry;
        if (k < nblk) blk[k] = carry + s[tid] - v;
        __syncthreads();
        if (tid == SCAN_THREADS - 1) s_carry = carry + s[tid];
        __syncthreads();
    }
    if (tid == 0) {
        if (total_a) total_a[0] = s_carry;
        if (total_b) total_b[0] = s_carry;
    }
}

// L[p] = 1 + the number of roots before p, for every root p.
__global__ void __launch_bounds__(LIN_THREADS) k_ccl_rank(const int *__restrict__ T, int npix, const int *__restrict__ blk_off, int *__restrict__ L)
{
    __shared__ int s_w[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long base = (long long)blockIdx.x * LIN_PIX;
    bool root[LIN_PER_THREAD];
    unsigned long long bal[LIN_PER_THREAD];
#pragma unroll
    for (int k = 0; k < LIN_PER_THREAD; k++) {
        const long long pl = base + k * LIN_THREADS + tid;
        root[k] = pl < npix && T[pl] == (int)pl;
        bal[k] = __ballot(root[k]);
        if (lane == 0) s_w[k * (LIN_THREADS / 64) + wave] = __popcll(bal[k]);
    }
    __syncthreads();
    int off = blk_off[blockIdx.x];
#pragma unroll
    for (int k = 0; k < LIN_PER_THREAD; k++) {
#pragma unroll
        for (int w = 0; w < LIN_THREADS / 64; w++) {
            const int c = s_w[k * (LIN_THREADS / 64) + w];
            if (w == wave && root[k]) L[base + k * LIN_THREADS + tid] = off + __popcll(bal[k] & ((1ull << lane) - 1ull)) + 1;
            off += c;
        }
    }
}

__device__ inline void area_table_add(int *keys, int *cnts, int key, int n)
{
    unsigned slot = ((unsigned)key * 2654435761u) >> 21; // 11 bits: HASH_SLOTS
    static_assert(HASH_SLOTS == 2048, "hash width");
    for (;;) {
        const int prev = atomicCAS(&keys[slot], 0, key);
        if (prev == 0 || prev == key) {
            atomicAdd(&cnts[slot], n);
            return;
        }
        slot = (slot + 1) & (HASH_SLOTS - 1); // at most LIN_PIX distinct keys: a free slot always exists
    }
}

// The area contribution of one wave-load of labels (0: none) to the table: the lanes that share the first label add once.
__device__ inline void area_table_wave(int *keys, int *cnts, int lab, int lane)
{
    const unsigned long long act = __ballot(lab > 0);
    if (act == 0) return;
    const int first = __ffsll((long long)act) - 1;
    const int lead = __shfl(lab, first, 64);
    const unsigned long long same = __ballot(lab == lead);
    if (lane == first) area_table_add(keys, cnts, lead, __popcll(same));
    else if (lab > 0 && lab != lead) area_table_add(keys, cnts, lab, 1);
}

// L[p] = the label of p's root (0: background); areas[l-1] += the block's pixels of label l, for l <= areas_cap (areas NULL: no count).
__global__ void __launch_bounds__(LIN_THREADS) k_ccl_relabel(const int *__restrict__ T, int npix, int *L, int *areas, int areas_cap)
{
    __shared__ int keys[HASH_SLOTS], cnts[HASH_SLOTS];
    const int tid = threadIdx.x, lane = tid & 63;
    const long long base = (long long)blockIdx.x * LIN_PIX;
    if (areas) {
        for (int k = tid; k < HASH_SLOTS; k += LIN_THREADS) {
            keys[k] = 0;
            cnts[k] = 0;
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < LIN_PER_THREAD; k++) {
        const long long pl = base + k * LIN_THREADS + tid;
        int lab = 0;
        if (pl < npix) {
            const int q = T[pl];
            if (q >= 0) lab = L[q]; // a root reads its own label, written by k_ccl_rank
            L[pl] = lab;
        }
        if (areas) area_table_wave(keys, cnts, lab, lane);
    }
    if (areas) {
        __syncthreads();
        for (int k = tid; k < HASH_SLOTS; k += LIN_THREADS) {
            const int key = keys[k];
            if (key > 0 && key - 1 < areas_cap) atomicAdd(&areas[key - 1], cnts[k]);
        }
    }
}

// (area, label) as one key whose maximum is the largest area and, among equals, the lowest label; 0: nothing.
__device__ inline unsigned long long area_key(int area, int label) { return ((unsigned long long)(unsigned)area << 32) | (0xffffffffu - (unsigned)label); }
__device__ inline int key_label(unsigned long long key) { return key ? (int)(0xffffffffu - (unsigned)(key & 0xffffffffu)) : 0; }
__device__ inline int key_area(unsigned long long key) { return (int)(key >> 32); }

__device__ inline unsigned long long wave_max_u64(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned hi = (unsigned)__shfl_xor((int)(v >> 32), d, 64), lo = (unsigned)__shfl_xor((int)(v & 0xffffffffu), d, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}

// best[0] = the label of the largest of areas[0..*num), best[1] = its area; {0, 0} when *num == 0.
__global__ void __launch_bounds__(ARG_THREADS) k_ccl_argmax(const int *__restrict__ areas, const int *__restrict__ num, int *__restrict__ best)
{
    __shared__ unsigned long long s_best[ARG_THREADS / 64];
    const int tid = threadIdx.x, n = num[0];
    unsigned long long key = 0;
    for (int k = tid; k < n; k += ARG_THREADS) {
        const unsigned long long c = area_key(areas[k], k + 1);
        key = c > key ? c : key;
    }
    key = wave_max_u64(key);
    if ((tid & 63) == 0) s_best[tid >> 6] = key;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < ARG_THREADS / 64; w++) key = s_best[w] > key ? s_best[w] : key;
        best[0] = key_label(key);
        best[1] = key_area(key);
    }
}

__global__ void __launch_bounds__(LIN_THREADS) k_ccl_select(const int *__restrict__ L, int npix, const int *__restrict__ best, const int *__restrict__ num,
                                                            float hi, float lo, float *__restrict__ out, int *__restrict__ num_out,
                                                            int *__restrict__ area_out)
{
    const long long base = (long long)blockIdx.x * LIN_PIX;
    const int b = best[0];
#pragma unroll
    for (int k = 0; k < LIN_PER_THREAD; k++) {
        const long long pl = base + k * LIN_THREADS + threadIdx.x;
        if (pl < npix) out[pl] = (b > 0 && L[pl] == b) ? hi : lo;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (num_out) num_out[0] = num[0];
        if (area_out) area_out[0] = best[1];
    }
}

// ---- the small form: everything in one workgroup's LDS -------------------------------------------------------------------------
// L_out, num_out, areas_out, sel_out and best_area_out may each be NULL.  sel_out may alias A: A is only read before the first
// barrier.  areas_out[num..areas_cap) is set to 0.
__global__ void __launch_bounds__(SMALL_THREADS) k_ccl_small(const float *A, int nrows, int ncols, int conn8, int npad, int *__restrict__ L_out,
                                                             int *__restrict__ num_out, int *__restrict__ areas_out, int areas_cap, float *sel_out,
                                                             float hi, float lo, int *__restrict__ best_area_out)
{
    extern __shared__ int ccl_lds[];
    int *L = ccl_lds, *C = ccl_lds + npad; // the forest; the area of a root, later its label
    volatile int *vL = L;
    __shared__ int s_w[SMALL_WAVES];
    __shared__ int s_carry;
    __shared__ unsigned long long s_best[SMALL_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, npix = nrows * ncols;
    if (tid == 0) s_carry = 0;

    // 1. every pixel points at the start of its vertical run; a run may span several 64-row chunks of its column
    for (int j = wave; j < ncols; j += SMALL_WAVES) {
        int carry = -1; // first row of the run that reaches the chunk's first row (-1: none does)
        for (int i0 = 0; i0 < nrows; i0 += 64) {
            const int i = i0 + lane, p = j * nrows + i;
            const bool fg = i < nrows && A[p] > 0.0f;
            const unsigned long long bal = __ballot(fg);
            if (i < nrows) {
                const unsigned long long below = ~bal & ((1ull << lane) - 1ull);
                const int st = below ? i0 + 64 - __clzll((long long)below) : (carry >= 0 ? carry : i0);
                L[p] = fg ? j * nrows + st : -1;
                C[p] = 0;
            }
            if (bal >> 63) {
                const unsigned long long z = ~bal;
                carry = z ? i0 + 64 - __clzll((long long)z) : (carry >= 0 ? carry : i0);
            } else {
                carry = -1;
            }
        }
    }
    __syncthreads();
    // 2. merge the runs of neighbouring columns
    for (int p = tid; p < npix; p += SMALL_THREADS) {
        const int j = p / nrows, i = p - j * nrows;
        if (j == 0 || vL[p] < 0) continue;
        west_rules(conn8 != 0,
                   [&](int di, int dj) { const int ii = i + di; return ii >= 0 && ii < nrows && vL[p + dj * nrows + di] >= 0; },
                   [&](int di) { lds_union(L, p, p - nrows + di); });
    }
    __syncthreads();
    // 3. flatten
    for (int p = tid; p < npix; p += SMALL_THREADS) {
        const int v = vL[p];
        if (v >= 0) vL[p] = lds_find(vL, v);
    }
    __syncthreads();
    // 4. areas, at the roots
    for (int base = 0; base < npix; base += SMALL_THREADS) {
        const int p = base + tid;
        const int r = p < npix ? L[p] : -1;
        const unsigned long long act = __ballot(r >= 0);
        if (act == 0) continue;
        const int first = __ffsll((long long)act) - 1;
        const int lead = __shfl(r, first, 64);
        const unsigned long long same = __ballot(r == lead);
        if (lane == first) atomicAdd(&C[lead], __popcll(same));
        else if (r >= 0 && r != lead) atomicAdd(&C[r], 1);
    }
    __syncthreads();
    // 5. rank the roots in memory order; a root's counter becomes its label
    unsigned long long best = 0;
    for (int base = 0; base < npix; base += SMALL_THREADS) {
        const int p = base + tid;
        const bool root = p < npix && L[p] == p;
        const unsigned long long bal = __ballot(root);
        if (lane == 0) s_w[wave] = __popcll(bal);
        __syncthreads();
        int off = s_carry;
        for (int w = 0; w < wave; w++) off += s_w[w];
        if (root) {
            const int rank = off + __popcll(bal & ((1ull << lane) - 1ull)), area = C[p];
            if (areas_out && rank < areas_cap) areas_out[rank] = area;
            const unsigned long long key = area_key(area, rank + 1);
            best = key > best ? key : best;
            C[p] = rank + 1;
        }
        __syncthreads();
        if (tid == 0) {
            int tot = 0;
            for (int w = 0; w < SMALL_WAVES; w++) tot += s_w[w];
            s_carry += tot;
        }
        __syncthreads();
    }
    // 6. the largest area, the lowest label on a tie
    best = wave_max_u64(best);
    if (lane == 0) s_best[wave] = best;
    __syncthreads();
    for (int w = 0; w < SMALL_WAVES; w++) best = s_best[w] > best ? s_best[w] : best;
    const int best_label = key_label(best), num = s_carry;
    // 7. the outputs
    for (int p = tid; p < npix; p += SMALL_THREADS) {
        const int r = L[p];
        const int lab = r >= 0 ? C[r] : 0;
        if (L_out) L_out[p] = lab;
        if (sel_out) sel_out[p] = (lab > 0 && lab == best_label) ? hi : lo;
    }
    if (areas_out)
        for (int k = num + tid; k < areas_cap; k += SMALL_THREADS) areas_out[k] = 0;
    if (tid == 0) {
        if (num_out) num_out[0] = num;
        if (best_area_out) best_area_out[0] = key_area(best);
    }
}

} // namespace ccl
} // namespace pdeip
