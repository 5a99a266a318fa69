// fanout_kernel.h -- fanout-limited gossip (gossip.h, gossip_engine_set_fanout): the selection rule
// and the per-tick thinning of the peer lists.
//
// The rule.  A Send from node u to peer v, copy c < mult(u -> v), made in tick T happens iff
//     lo = min(u, v), hi = max(u, v)
//     x  = Philox4x32-10(counter = (lo, hi, (uint32)T, c), key = (seed & 0xffffffff, (seed >> 32) ^ "FANO"))
//     w  = u < v ? x[0] : x[1]                 (one Philox call serves both directions of a link)
//     selected = thr[u] == 0xffffffff || w < thr[u]
// The draw belongs to (sender, receiver, copy, tick), not to a share: everything a node sends in one
// tick shares it (the round-based push model), so it is the same for all 64 columns of a frontier
// word and the pull kernels need no change -- they walk a thinned CSR.
//
// Per tick T, after the tick's births and before the frontier buffers flip (engine.hip fanout_launch):
//   k_fanout_count    pass 1.  A wave owns 64 consecutive nodes and strides the flat entry range
//                     [rowptr[c0], rowptr[c0 + 64)) of their rows, 64 entries a step, aligned to 64
//                     entries so that one ballot is one word of the selection bitmap.  Per entry j of
//                     row v (peer u = col[j]): in side, any copy u -> v selected (sender threshold
//                     in_thr[j] and multiplicities emult[j] precomputed on the host: no gather);
//                     out side, the number of selected copies v -> u.  Per node: the in-count, and
//                     sent_f[v] += out-count x (first receptions + generations of v in T).
//   (exclusive scan)  hipcub::DeviceScan over the in-counts -> rowptr_t (int64, n + 1)
//   k_fanout_compact  pass 2.  The same walk over the bitmap: selected entry j goes to
//                     col_t[rowptr_t[c0] + rank of j among the selected entries of the wave's range]
//                     -- rows are contiguous and in order, so the compaction is stable and needs no
//                     per-entry row lookup.
// Tick T + 1's k_pull launches read (rowptr_t, col_t) where they read (rowptr, col) in a flood.
#pragma once

#include <stdint.h>

#include "philox.h"

namespace gossip {

constexpr uint32_t kFanoutKey1 = 0x46414E4Fu;   // "FANO": xor of the second key word
constexpr uint32_t kFanoutAlways = 0xffffffffu;  // threshold: forward with probability 1

// x[0], x[1] of the link {a, b} (either order), copy c, tick T
GOSSIP_HD void fanout_draw(uint64_t seed, uint32_t a, uint32_t b, uint32_t c, uint32_t tick, uint32_t x[2]) {
    uint32_t ctr[4] = {a < b ? a : b, a < b ? b : a, tick, c};
    philox4x32_10(ctr, (uint32_t)seed, (uint32_t)(seed >> 32) ^ kFanoutKey1);
    x[0] = ctr[0];
    x[1] = ctr[1];
}
GOSSIP_HD bool fanout_pass(uint32_t w, uint32_t thr) { return thr == kFanoutAlways || w < thr; }
// THE definition of the rule: Send u -> v, copy c, in tick T, sender threshold thr
GOSSIP_HD bool fanout_selected(uint64_t seed, uint32_t u, uint32_t v, uint32_t c, uint32_t tick, uint32_t thr) {
    uint32_t x[2];
    fanout_draw(seed, u, v, c, tick, x);
    return fanout_pass(u < v ? x[0] : x[1], thr);
}
// gossip_engine_set_fanout: expected fanout k of a node with deg peer copies (binomial, not an exact
// k-subset: that needs v's position in u's list and u's degree per entry, two more gathers)
GOSSIP_HD uint32_t fanout_threshold(uint32_t k, uint32_t deg) {
    return deg <= k ? kFanoutAlways : (uint32_t)(((uint64_t)k << 32) / deg);
}

#if defined(__HIPCC__)

constexpr uint32_t kFanoutStatLine = 16, kFanoutStatReplicas = 64;  // 128-B lines of [selected_in, selected_out]

struct FanoutArgs {
    const int64_t* rowptr;   // the full graph
    const int32_t* col;
    const uint32_t* in_thr;  // per entry j of row v: thr[col[j]]
    const uint8_t* emult;    // per entry: mult(col[j] -> v) | mult(v -> col[j]) << 4
    const uint32_t* thr;     // per node
    const uint32_t* recv;
    const uint32_t* gen;
    uint32_t* recv_prev;
    uint32_t* gen_prev;
    unsigned long long* sent_f;
    unsigned long long* bitmap;  // bit j: entry j selected (zeroed before pass 1)
    uint32_t* cnt;               // per node: selected entries (cnt[n] stays 0)
    const int64_t* rowptr_t;     // pass 2
    int32_t* col_t;
    unsigned long long* stat;
    uint64_t seed;
    uint32_t tick;
    uint32_t n;
};

__global__ __launch_bounds__(256) void k_fanout_count(FanoutArgs a) {
    __shared__ uint32_t s_off[4][65], s_thr[4][64], s_in[4][64], s_out[4][64];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t nch = ((uint64_t)a.n + 63u) / 64u;
    unsigned long long tin = 0ull, tout = 0ull;
    for (uint64_t ch = (uint64_t)blockIdx.x * 4u + wv; ch < nch; ch += (uint64_t)gridDim.x * 4u) {
        const uint64_t c0 = ch * 64u, v = c0 + lane;
        const int64_t rp0 = a.rowptr[c0];
        const uint32_t len = (uint32_t)(a.rowptr[c0 + 64u < a.n ? c0 + 64u : a.n] - rp0);
        s_off[wv][lane] = (uint32_t)(a.rowptr[v < a.n ? v : a.n] - rp0);
        if (lane == 0) s_off[wv][64] = len;
        s_thr[wv][lane] = v < a.n ? a.thr[v] : 0u;
        s_in[wv][lane] = 0u;
        s_out[wv][lane] = 0u;
        __builtin_amdgcn_wave_barrier();
        const uint32_t head = (uint32_t)(rp0 & 63);
        const int64_t j0 = rp0 - head;  // 64-aligned
        for (uint32_t base = 0; base < head + len; base += 64u) {
            const uint32_t jj = base + lane;
            bool sel = false;
            if (jj >= head && jj < head + len) {
                const uint32_t rel = jj - head;
                const int64_t j = j0 + jj;
                const uint32_t u = (uint32_t)a.col[j], ti = a.in_thr[j], m = a.emult[j];
                uint32_t i = 0;  // the row: the last i in [0, 63] with s_off[i] <= rel
#pragma unroll
                for (uint32_t s = 32; s; s >>= 1)
                    if (s_off[wv][i + s] <= rel) i += s;
                const uint32_t vv = (uint32_t)c0 + i, to = s_thr[wv][i];
                const uint32_t mi = m & 15u, mo = m >> 4, mm = mi > mo ? mi : mo;
                uint32_t oc = 0;
                for (uint32_t c = 0; c < mm; c++) {
                    uint32_t x[2];
                    fanout_draw(a.seed, vv, u, c, a.tick, x);
                    const uint32_t w_out = vv < u ? x[0] : x[1], w_in = u < vv ? x[0] : x[1];
                    oc += (c < mo && fanout_pass(w_out, to)) ? 1u : 0u;
                    sel |= c < mi && fanout_pass(w_in, ti);
                }
                if (oc) atomicAdd(&s_out[wv][i], oc);
                if (sel) atomicAdd(&s_in[wv][i], 1u);
            }
            const unsigned long long bal = __ballot(sel);
            if (lane == 0) {
                // a word the range covers only in part is shared with the neighbouring waves
                unsigned long long* wp = a.bitmap + ((j0 + base) >> 6);
                if (base < head || base + 64u > head + len) {
                    if (bal) atomicOr(wp, bal);
                } else {
                    *wp = bal;
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        if (v < a.n) {
            const uint32_t ic = s_in[wv][lane], oc = s_out[wv][lane];
            const uint32_t r = a.recv[v], g = a.gen[v];
            const uint32_t d = (r - a.recv_prev[v]) + (g - a.gen_prev[v]);
            if (d && oc) a.sent_f[v] += (unsigned long long)oc * d;
            a.recv_prev[v] = r;
            a.gen_prev[v] = g;
            a.cnt[v] = ic;
            tin += ic;
            tout += oc;
        }
        __builtin_amdgcn_wave_barrier();
    }
    for (int off = 32; off > 0; off >>= 1) {
        tin += __shfl_xor(tin, off, 64);
        tout += __shfl_xor(tout, off, 64);
    }
    if (lane == 0) {
        unsigned long long* st = a.stat + (blockIdx.x & (kFanoutStatReplicas - 1u)) * kFanoutStatLine;
        if (tin) atomicAdd(st, tin);
        if (tout) atomicAdd(st + 1, tout);
    }
}

__global__ __launch_bounds__(256) void k_fanout_compact(FanoutArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t nch = ((uint64_t)a.n + 63u) / 64u;
    for (uint64_t ch = (uint64_t)blockIdx.x * 4u + wv; ch < nch; ch += (uint64_t)gridDim.x * 4u) {
        const uint64_t c0 = ch * 64u;
        const int64_t rp0 = a.rowptr[c0];
        const uint32_t len = (uint32_t)(a.rowptr[c0 + 64u < a.n ? c0 + 64u : a.n] - rp0);
        const uint32_t head = (uint32_t)(rp0 & 63);
        const int64_t j0 = rp0 - head;
        int64_t out = a.rowptr_t[c0];
        for (uint32_t base = 0; base < head + len; base += 64u) {
            unsigned long long w = a.bitmap[(j0 + base) >> 6];
            const uint32_t lo = base < head ? head - base : 0u;  // (base 0 only)
            const uint32_t hi = head + len - base < 64u ? head + len - base : 64u;
            w &= (hi == 64u ? ~0ull : (1ull << hi) - 1ull) & ~((1ull << lo) - 1ull);
            if ((w >> lane) & 1ull) a.col_t[out + __popcll(w & ((1ull << lane) - 1ull))] = a.col[j0 + base + lane];
            out += __popcll(w);
        }
    }
}

// sum of a 64-bit per-node counter into *out (edge_events in fanout mode: sent_f)
__global__ __launch_bounds__(256) void k_sum_u64(const unsigned long long* a, uint32_t n, unsigned long long* out) {
    unsigned long long s = 0;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) s += a[i];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(out, s);
}

#endif  // __HIPCC__

}  // namespace gossip
