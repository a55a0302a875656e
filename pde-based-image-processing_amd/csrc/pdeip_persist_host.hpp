// pdeip_persist_host.hpp -- host side of the one-launch exact-order walkers (k_sor_exact_persist, k_pde8_exact_persist): the
// schedule table, the control block and the mailbox of a call.
//
// Control block (ws[WS_CTL], cleared by every call from word 1 on: k_persist_setup):
//   word 0        abort (sticky: cleared only by pdeip_persist_error(), so a timed-out wait cannot be lost under the next call's reset)
//   words 4..11   one ticket counter per XCD list
//   words 16..    progress counters [nframes][iter][B]
//   128-byte aligned behind them: the west-edge mailbox
// Schedule table (ws[WS_ORDER], built by every call on its stream): ints 0..8 = offsets of eight lists into the items, ints 9..10 =
// the stamp B, T of the table the buffer holds, items from int 16 on, an item = b | (t << 16).  Every list is sorted by
// key = b + 2t, in which every dependency of an item -- (b-1,t), (b,t-1), (b+1,t-1) -- has a smaller key.
//   The host keeps no record of what the buffer holds: a captured HIP graph carries a k_persist_setup node that rewrites it on every
//   replay without the host's knowing, so a shape remembered on the host can be stale (eager X, replay Y, eager X walked Y's table).
//   The walkers compare the stamp with their own (B, T) before they take an item (persist_take_item) and raise the abort word on a
//   mismatch instead of walking somebody else's table.
//   XCD-affine (opt-in, PDEIP_PERSIST_XCD=1, and only when grid <= compute units): list x holds the strips b = x (mod 8),
//   all their sweeps; a workgroup takes the next item of the list of the XCD it runs on (HW_REG_XCC_ID) and only steals
//   from the other lists when its own is used up.  The sweeps of a strip then follow each other through ONE L2: sweep t+1 reads
//   the packed coefficients sweep t fetched 10-15 us earlier.  With every workgroup resident and exactly one item per
//   workgroup every item is taken by a running workgroup, whatever the placement: placement changes speed only.
//   Default (and always with more workgroups than compute units): one list in key order -- a running workgroup then only ever
//   waits for items with smaller tickets, which are running or finished: live for any grid, any dispatch order and whatever
//   other kernels hold compute units.
#pragma once
#include "pdeip_ctx.hpp"
#include "pdeip_sor_exact.hpp"

namespace pdeip {

constexpr int PERSIST_HDR_WORDS = 16, PERSIST_TABLE_HDR = 16;

// Schedule table on the device.  Thread (b, t) writes its item at its rank in its list: the number of items of the list that
// come before it in (key, t) order, key = b + 2t.  Items (b', t') of list x: 0 <= b' < B, b' = x (mod 8) when affine.
static __device__ __forceinline__ int persist_count_below(int lim, int B, int affine, int x)
{ // #{b' in [0, min(lim, B)) : affine ? b' % 8 == x : true}
    int n = lim < B ? lim : B;
    if (n <= 0) return 0;
    return affine ? (n - x + 7) / 8 : n;
}
static __device__ __forceinline__ void persist_order_thread(int *table, int idx, int B, int T, int affine)
{
    if (idx < PERSIST_TABLE_HDR) { // list offsets: list x starts behind the items of the lists before it
        int off = 0;
        for (int x = 0; x < idx && x < 8; x++) off += (affine ? (B - x + 7) / 8 : (x == 0 ? B : 0)) * T;
        const int stamp = idx == PERSIST_STAMP_B ? B : (idx == PERSIST_STAMP_T ? T : 0); // what the walkers check (persist_take_item)
        table[idx] = idx <= 8 ? (idx == 8 ? B * T : off) : stamp;
    }
    if (idx >= B * T) return;
    const int b = idx % B, t = idx / B, key = b + 2 * t, x = affine ? (b & 7) : 0;
    int rank = 0;
    for (int tt = 0; tt < T; tt++) {
        // items of sweep tt with a smaller key, or the same key and a smaller sweep: b' < key - 2 tt (+1 when tt < t)
        rank += persist_count_below(key - 2 * tt + (tt < t ? 1 : 0), B, affine, x);
    }
    int first = 0;
    for (int xx = 0; xx < x; xx++) first += ((B - xx + 7) / 8) * T;
    table[PERSIST_TABLE_HDR + first + rank] = b | (t << 16);
}
static __global__ void k_persist_order(int *table, int B, int T, int affine) // the table alone (pdeip_debug_persist_order)
{
    persist_order_thread(table, (int)(blockIdx.x * blockDim.x + threadIdx.x), B, T, affine);
}
// What every call launches in front of its walker: clears the control block and the mailbox (words 1 .. n-1; word 0 is the sticky
// abort word) and builds the call's schedule table, in ONE launch -- the table costs a call no launch of its own.  A kernel rather
// than hipMemsetAsync: an exact-order call captured into a HIP graph replayed with stale counters when the clear was a memset
// node.  The host sizes the grid by whichever is larger, the words or the table.
static __global__ void k_persist_setup(unsigned *words, size_t n, int *table, int B, int T, int affine)
{
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid + 1 < n) words[gid + 1] = 0u;
    const size_t nt = (size_t)B * T > (size_t)PERSIST_TABLE_HDR ? (size_t)B * T : (size_t)PERSIST_TABLE_HDR;
    if (gid < nt) persist_order_thread(table, (int)gid, B, T, affine);
}

inline int persist_prepare(hipStream_t s, int B, int iter, int nframes, size_t mail_bytes, PersistCtl *ctl)
{
    const size_t nprog = (size_t)nframes * iter * B;
    const size_t ctl_bytes = ((PERSIST_HDR_WORDS + nprog) * sizeof(unsigned) + 127) / 128 * 128;
    float *ctl_f = nullptr, *order_f = nullptr;
    RC(ws_get(WS_CTL, ctl_bytes + mail_bytes, &ctl_f));
    RC(ws_get(WS_ORDER, (PERSIST_TABLE_HDR + (size_t)B * iter) * sizeof(int), &order_f));
    const int cus = device_cus();
    // Default: the single key-ordered list -- a running workgroup only ever waits for smaller tickets, which are running or
    // finished, whatever else holds compute units.  The XCD-affine lists (3-5 % faster at 4K) are live only while every
    // workgroup of the grid is resident, which a library inside somebody else's process cannot know: opt-in, PDEIP_PERSIST_XCD=1.
    const int affine = (env_int("PDEIP_PERSIST_XCD", 0) != 0 && nprog <= (size_t)(cus > 0 ? cus : 1)) ? 1 : 0;
    {
        // The table is built by every call, on the call's stream, by a plain launch (capturable into a HIP graph): whatever ran on the
        // device since the host last looked -- a replayed graph rewrites this buffer -- the walker launched next finds its own table.
        // It shares its launch with the clear of the control block and the mailbox.
        const size_t nwords = (ctl_bytes + mail_bytes) / sizeof(unsigned);
        const size_t nitems = (size_t)B * iter > (size_t)PERSIST_TABLE_HDR ? (size_t)B * iter : (size_t)PERSIST_TABLE_HDR;
        const size_t nthreads = nwords > nitems ? nwords : nitems;
        hipLaunchKernelGGL(k_persist_setup, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, s, reinterpret_cast<unsigned *>(ctl_f), nwords,
                           reinterpret_cast<int *>(order_f), B, iter, affine);
        HIPCHK(hipGetLastError());
    }
    ctl->abort_flag = reinterpret_cast<unsigned *>(ctl_f);
    ctl->ticket = ctl->abort_flag + 4;
    ctl->progress = ctl->abort_flag + PERSIST_HDR_WORDS;
    ctl->order = reinterpret_cast<const int *>(order_f);
    ctl->mail = reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(ctl_f) + ctl_bytes);
    cur_dev()->persist_used = true;
    return PDEIP_OK;
}

} // namespace pdeip
