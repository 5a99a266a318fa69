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
//
// Fault injection (gossip.h, gossip_engine_set_outages / _set_link_loss) is a second reason to drop an
// entry in the same pass: k_fanout_count_faults is the count pass with three additions.  Entry (row v,
// peer u) survives iff v is up in tick T + 1 and some copy c < mult(u -> v) has fanout_pass && !lost,
//     y = Philox4x32-10(counter = (lo, hi, (uint32)T, c), key = (seed & 0xffffffff, (seed >> 32) ^ "LOSS"))
//     lost = loss_thr == 0xffffffff || (u < v ? y[0] : y[1]) < loss_thr        (u the sender)
// with a seed of its own.  "v is down in T + 1" is a search of v's merged outage intervals (a per-node
// CSR, outage_down below), decided once per node in the chunk prologue and kept in LDS next to s_thr; no
// state is carried from tick to tick.  The out side is unchanged: a Send to a down node or a lost Send is
// made and counted.  k_fanout_count stays the code it was (one body, two instantiations).
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


constexpr uint32_t kLossKey1 = 0x4C4F5353u;  // "LOSS": xor of the second key word of the loss draw

// y[0], y[1] of the link {a, b} (either order), copy c, tick T
GOSSIP_HD void loss_draw(uint64_t seed, uint32_t a, uint32_t b, uint32_t c, uint32_t tick, uint32_t y[2]) {
    uint32_t ctr[4] = {a < b ? a : b, a < b ? b : a, tick, c};
    philox4x32_10(ctr, (uint32_t)seed, (uint32_t)(seed >> 32) ^ kLossKey1);
    y[0] = ctr[0];
    y[1] = ctr[1];
}
GOSSIP_HD bool loss_pass(uint32_t w, uint32_t thr) { return thr == 0xffffffffu || w < thr; }
// THE definition of the loss rule: is the Send u -> v, copy c, made in tick T lost?
GOSSIP_HD bool fault_lost(uint64_t seed, uint32_t u, uint32_t v, uint32_t c, uint32_t tick, uint32_t thr) {
    uint32_t y[2];
    loss_draw(seed, u, v, c, tick, y);
    return loss_pass(u < v ? y[0] : y[1], thr);
}
// THE definition of "node v is down in tick t": its merged, ascending, disjoint intervals are
// [from[k], to[k]) for k in [off[v], off[v + 1]); the last one that starts at or before t decides
GOSSIP_HD bool outage_down(const uint32_t* off, const uint32_t* from, const uint32_t* to, uint32_t v, uint64_t t) {
    const uint32_t first = off[v];
    uint32_t lo = first, hi = off[v + 1];
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (from[mid] <= t) lo = mid + 1u;
        else hi = mid;
    }
    return lo > first && t < to[lo - 1u];
}

// ---- exact-k fanout (gossip.h, gossip_engine_set_fanout_exact / _set_fanout_counts) ---------------
// Sender u with D out-copies and fanout count k[u] in tick T: every out-copy (v, c) gets the 64-bit draw
//     x = Philox4x32-10(counter = (lo, hi, (uint32)T, c), key = (seed & 0xffffffff, (seed >> 32) ^ "FANK"))
//     w(u -> v, c, T) = u < v ? x[0] << 32 | x[1] : x[2] << 32 | x[3]
// and the copies with the k[u] smallest draws are sent: q(u, T) = the k[u]-th smallest of the D draws,
//     selected = k[u] > 0 && (D <= k[u] || w <= q(u, T))
// i.i.d. draws ranked: a uniform k-subset.  Draws that tie at q are all selected (the out-count is counted).
// Per tick T, in front of the count pass:
//   k_fanout_kth      one lane per row u.  A node that must select (D > k[u] >= 1) walks its row, draws once
//                     per out-copy and keeps the k smallest in LDS ([slot][lane]: conflict-free), the largest
//                     of them and its slot in registers; a draw below the largest replaces it and costs one
//                     re-scan of the k slots (about k ln(D / k) of them per row).  It writes bound[u] = q and
//                     owns the out side: sent_f[u] += out-count x (first receptions + generations of u in T),
//                     and rolls recv_prev / gen_prev (the exact count pass does not touch them).  A node that
//                     sends every copy (D <= k[u]) or none (k[u] = 0) makes no draw: bound = all-ones, out-count
//                     from the setter's table.
//   count pass        fanout_count_body<FAULTS, true>: the in side is c < mi && w(u -> v, c, T) <= bound[u],
//                     bound gathered by col[j] (n x 8 B: cache-resident).  The 2^64 + 1 predicates "none" and
//                     "w <= q" do not fit 64 bits: a silent sender (k[u] = 0) is taken out at the setter, which
//                     writes in-multiplicity 0 for its entries, so the table needs no "none"; "all" is
//                     2^64 - 1, which w <= bound passes exactly.
//   scan, k_fanout_compact   unchanged.
constexpr uint32_t kFanoutExactKey1 = 0x46414E4Bu;  // "FANK": xor of the second key word of the exact draw
constexpr uint32_t kFanoutExactMax = 32;            // largest k at a node that must select (LDS slots per lane)
constexpr uint64_t kFanoutExactAll = ~0ull;         // bound: every copy passes

// the draw's four words -> w of direction u -> v
GOSSIP_HD uint64_t fanout_exact_word(uint32_t u, uint32_t v, const uint32_t x[4]) {
    return u < v ? ((uint64_t)x[0] << 32 | x[1]) : ((uint64_t)x[2] << 32 | x[3]);
}
// w(u -> v, c, T)
GOSSIP_HD uint64_t fanout_exact_draw(uint64_t seed, uint32_t u, uint32_t v, uint32_t c, uint32_t tick) {
    uint32_t ctr[4] = {u < v ? u : v, u < v ? v : u, tick, c};
    philox4x32_10(ctr, (uint32_t)seed, (uint32_t)(seed >> 32) ^ kFanoutExactKey1);
    return fanout_exact_word(u, v, ctr);
}
// THE compare: plain <= on all 64 bits, so exact at w = 0 (passes every bound), at w = 2^64 - 1 (passes
// only the bound 2^64 - 1) and for kFanoutExactAll
GOSSIP_HD bool fanout_exact_pass(uint64_t w, uint64_t bound) { return w <= bound; }
// The k smallest of a stream of draws: keep[] holds them (any order), mx the largest of them, at, its slot,
// ties the draws seen outside keep[] that equal mx.  keep[i * stride] is slot i (the kernel's [slot][lane]).
struct FanoutExactTop {
    uint64_t mx;
    uint32_t at, have, ties;
};
GOSSIP_HD void fanout_exact_push(FanoutExactTop& s, uint64_t* keep, uint32_t stride, uint32_t k, uint64_t w) {
    if (s.have < k) {
        keep[(size_t)s.have * stride] = w;
        if (s.have == 0 || w > s.mx) {
            s.mx = w;
            s.at = s.have;
        }
        s.have++;
    } else if (w < s.mx) {
        const uint64_t old = s.mx;
        keep[(size_t)s.at * stride] = w;
        uint64_t m = 0;
        uint32_t at = 0;
        for (uint32_t i = 0; i < k; i++) {
            const uint64_t x = keep[(size_t)i * stride];
            if (x >= m) {
                m = x;
                at = i;
            }
        }
        s.mx = m;
        s.at = at;
        s.ties = m == old ? s.ties + 1u : 0u;  // the evicted draw: still at the bound, or above it with every earlier tie
    } else if (w == s.mx) {
        s.ties++;
    }
}
// The bound of a sender with the draws w[0 .. D) and the count k: q = the k-th smallest (with multiplicity)
// if it must select (D > k >= 1), kFanoutExactAll if D <= k; *count = the copies sent (k, or more when draws
// tie at q; D; 0 at k = 0, where the bound means nothing: no copy is sent).  keep: min(k, D) words of scratch.
GOSSIP_HD uint64_t fanout_exact_bound(const uint64_t* w, uint32_t D, uint32_t k, uint64_t* keep, uint32_t* count) {
    if (k == 0u || D <= k) {
        *count = k ? D : 0u;
        return kFanoutExactAll;
    }
    FanoutExactTop s = {0ull, 0u, 0u, 0u};
    for (uint32_t i = 0; i < D; i++) fanout_exact_push(s, keep, 1u, k, w[i]);
    *count = s.have + s.ties;
    return s.mx;
}
// THE definition of the rule for one sender's D out-copies (receiver[i], copy[i]): selected[i], and the draws
// if asked for.  Returns the number selected.  Any k; D <= k and k = 0 make no selection.
inline uint32_t fanout_exact_row(uint64_t seed, uint32_t sender, uint32_t D, const uint32_t* receiver, const uint32_t* copy,
                                 uint32_t k, uint32_t tick, uint8_t* selected, uint64_t* draws, uint64_t* work /* D + min(k, D) */) {
    for (uint32_t i = 0; i < D; i++) {
        work[i] = fanout_exact_draw(seed, sender, receiver[i], copy[i], tick);
        if (draws) draws[i] = work[i];
    }
    uint32_t count = 0;
    const uint64_t bound = fanout_exact_bound(work, D, k, work + D, &count);
    for (uint32_t i = 0; i < D; i++) selected[i] = (k && fanout_exact_pass(work[i], bound)) ? 1 : 0;
    return count;
}

#if defined(__HIPCC__)

// 128-B lines of [selected_in, selected_out, lost_copies, down_copies, down_node_ticks] (the last three: faults)
constexpr uint32_t kFanoutStatLine = 16, kFanoutStatReplicas = 64;

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

// The two draws of the count pass with faults: fanout_draw (key1 = kFanoutKey1) and loss_draw (kLossKey1)
// with their round keys formed round by round.  Left to itself the compiler hoists the 20 round keys of
// each draw into SGPRs for the whole kernel; the 40, with the multipliers and the arguments, do not fit
// the 102 and spill into VGPR lanes.  The empty asm makes each round's keys a value it cannot precompute:
// two scalar adds per round, no spill.
__device__ __forceinline__ void draw_rolling(uint64_t seed, uint32_t key1, uint32_t a, uint32_t b, uint32_t c, uint32_t tick,
                                             uint32_t y[2]) {
    uint32_t x[4] = {a < b ? a : b, a < b ? b : a, tick, c};
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32) ^ key1;
#pragma unroll
    for (int r = 0; r < 10; r++) {
        asm volatile("" : "+s"(k0), "+s"(k1));
        philox4x32_round(x, k0, k1);
        k0 += kPhiloxW0;
        k1 += kPhiloxW1;
    }
    y[0] = x[0];
    y[1] = x[1];
}

struct FaultArgs {
    const uint32_t* out_off;   // n + 1: node v's outage intervals are [out_off[v], out_off[v + 1])
    const uint32_t* out_from;  // ticks, merged and ascending per node
    const uint32_t* out_to;
    uint64_t loss_seed;
    uint32_t loss_thr;         // 0: no loss, and no loss draw
};

// exact-k fanout: what k_fanout_kth and the exact count passes take on top of FanoutArgs
struct ExactArgs {
    const uint32_t* kx;    // per node: k[u] if u must select (D > k[u] >= 1), else 0
    const uint32_t* xout;  // per node: the out-count of a node that does not select (D, or 0 if silent)
    uint64_t* bound;       // per node: q(u, T), or kFanoutExactAll; written by k_fanout_kth each tick
};

template <bool FAULTS, bool EXACT>
__device__ __forceinline__ void fanout_count_body(const FanoutArgs a, const FaultArgs f, const ExactArgs xa) {
    __shared__ uint32_t s_off[4][65], s_thr[EXACT ? 1 : 4][EXACT ? 1 : 64], s_in[4][64], s_out[EXACT ? 1 : 4][EXACT ? 1 : 64];
    __shared__ uint32_t s_down[FAULTS ? 4 : 1][FAULTS ? 64 : 1];  // (faults) the row is down in tick + 1
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t nch = ((uint64_t)a.n + 63u) / 64u;
    unsigned long long tin = 0ull, tout = 0ull;
    uint32_t tlost = 0u, tdownc = 0u, tdown = 0u;  // (faults) this lane's lost copies, copies into down rows, down nodes
    const bool loss_on = FAULTS && f.loss_thr != 0u;  // uniform: a scalar branch
    for (uint64_t ch = (uint64_t)blockIdx.x * 4u + wv; ch < nch; ch += (uint64_t)gridDim.x * 4u) {
        const uint64_t c0 = ch * 64u, v = c0 + lane;
        const int64_t rp0 = a.rowptr[c0];
        const uint32_t len = (uint32_t)(a.rowptr[c0 + 64u < a.n ? c0 + 64u : a.n] - rp0);
        s_off[wv][lane] = (uint32_t)(a.rowptr[v < a.n ? v : a.n] - rp0);
        if (lane == 0) s_off[wv][64] = len;
        if constexpr (!EXACT) s_thr[wv][lane] = v < a.n ? a.thr[v] : 0u;
        if constexpr (FAULTS) {
            const bool dn = v < a.n && outage_down(f.out_off, f.out_from, f.out_to, (uint32_t)v, (uint64_t)a.tick + 1u);
            s_down[wv][lane] = dn ? 1u : 0u;
            tdown += dn ? 1u : 0u;
        }
        s_in[wv][lane] = 0u;
        if constexpr (!EXACT) s_out[wv][lane] = 0u;
        __builtin_amdgcn_wave_barrier();
        const uint32_t head = (uint32_t)(rp0 & 63);
        const int64_t j0 = rp0 - head;  // 64-aligned
        for (uint32_t base = 0; base < head + len; base += 64u) {
            const uint32_t jj = base + lane;
            bool sel = false;
            if (jj >= head && jj < head + len) {
                const uint32_t rel = jj - head;
                const int64_t j = j0 + jj;
                const uint32_t u = (uint32_t)a.col[j], ti = EXACT ? 0u : a.in_thr[j], m = a.emult[j];
                uint32_t i = 0;  // the row: the last i in [0, 63] with s_off[i] <= rel
#pragma unroll
                for (uint32_t s = 32; s; s >>= 1)
                    if (s_off[wv][i + s] <= rel) i += s;
                const uint32_t vv = (uint32_t)c0 + i, to = EXACT ? 0u : s_thr[wv][i];
                const uint32_t mi = m & 15u, mo = m >> 4, mm = mi > mo ? mi : mo;
                uint32_t oc = 0;
                if constexpr (EXACT) {  // the in side only: the sender's bound of this tick (k_fanout_kth), one gather
                    const uint64_t bd = xa.bound[u];
                    const bool rdown = FAULTS && s_down[FAULTS ? wv : 0u][FAULTS ? i : 0u] != 0u;
                    for (uint32_t c = 0; c < mi; c++) {  // (a silent sender's mi is 0: the setter)
                        const bool arrives = fanout_exact_pass(fanout_exact_draw(a.seed, u, vv, c, a.tick), bd);
                        bool lost = false;
                        if (loss_on) {
                            uint32_t y[2];
                            draw_rolling(f.loss_seed, kLossKey1, vv, u, c, a.tick, y);
                            lost = loss_pass(u < vv ? y[0] : y[1], f.loss_thr);
                        }
                        if constexpr (FAULTS) {
                            tdownc += (arrives && rdown) ? 1u : 0u;
                            tlost += (arrives && !rdown && lost) ? 1u : 0u;
                        }
                        sel |= arrives && !rdown && !lost;
                    }
                } else if constexpr (!FAULTS) {
                    for (uint32_t c = 0; c < mm; c++) {
                        uint32_t x[2];
                        fanout_draw(a.seed, vv, u, c, a.tick, x);
                        const uint32_t w_out = vv < u ? x[0] : x[1], w_in = u < vv ? x[0] : x[1];
                        oc += (c < mo && fanout_pass(w_out, to)) ? 1u : 0u;
                        sel |= c < mi && fanout_pass(w_in, ti);
                    }
                } else {
                    const bool rdown = s_down[wv][i] != 0u;
                    // a faults-only flood: both thresholds pass whatever the word, so the fanout draw is not made
                    const bool draw = to != kFanoutAlways || ti != kFanoutAlways;
                    for (uint32_t c = 0; c < mm; c++) {
                        uint32_t x[2] = {0u, 0u};
                        if (draw) draw_rolling(a.seed, kFanoutKey1, vv, u, c, a.tick, x);
                        const uint32_t w_out = vv < u ? x[0] : x[1], w_in = u < vv ? x[0] : x[1];
                        oc += (c < mo && fanout_pass(w_out, to)) ? 1u : 0u;  // made and counted, whatever becomes of it
                        const bool arrives = c < mi && fanout_pass(w_in, ti);  // the copy u -> vv was made
                        bool lost = false;
                        if (loss_on) {  // (not per lane "if it arrives": a wave's 64 lanes never all agree on that)
                            uint32_t y[2];
                            draw_rolling(f.loss_seed, kLossKey1, vv, u, c, a.tick, y);
                            lost = loss_pass(u < vv ? y[0] : y[1], f.loss_thr);
                        }
                        tdownc += (arrives && rdown) ? 1u : 0u;
                        tlost += (arrives && !rdown && lost) ? 1u : 0u;
                        sel |= arrives && !rdown && !lost;
                    }
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
            const uint32_t ic = s_in[wv][lane];
            if constexpr (!EXACT) {  // (exact: k_fanout_kth owns the out side and rolls the copies)
                const uint32_t oc = s_out[wv][lane];
                const uint32_t r = a.recv[v], g = a.gen[v];
                const uint32_t d = (r - a.recv_prev[v]) + (g - a.gen_prev[v]);
                if (d && oc) a.sent_f[v] += (unsigned long long)oc * d;
                a.recv_prev[v] = r;
                a.gen_prev[v] = g;
                tout += oc;
            }
            a.cnt[v] = ic;
            tin += ic;
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
    if constexpr (FAULTS) {
        unsigned long long fl = tlost, fc = tdownc, fd = tdown;
        for (int off = 32; off > 0; off >>= 1) {
            fl += __shfl_xor(fl, off, 64);
            fc += __shfl_xor(fc, off, 64);
            fd += __shfl_xor(fd, off, 64);
        }
        if (lane == 0) {
            unsigned long long* st = a.stat + (blockIdx.x & (kFanoutStatReplicas - 1u)) * kFanoutStatLine;
            if (fl) atomicAdd(st + 2, fl);
            if (fc) atomicAdd(st + 3, fc);
            if (fd) atomicAdd(st + 4, fd);
        }
    }
}

__global__ __launch_bounds__(256) void k_fanout_count(FanoutArgs a) { fanout_count_body<false, false>(a, FaultArgs{}, ExactArgs{}); }
// the count pass with faults: down rows select nothing, a lost copy selects nothing
__global__ __launch_bounds__(256) void k_fanout_count_faults(FanoutArgs a, FaultArgs f) { fanout_count_body<true, false>(a, f, ExactArgs{}); }
// the count passes of exact-k fanout: the in side against the senders' bounds, no out side
__global__ __launch_bounds__(256) void k_fanout_count_exact(FanoutArgs a, ExactArgs xa) { fanout_count_body<false, true>(a, FaultArgs{}, xa); }
__global__ __launch_bounds__(256) void k_fanout_count_exact_faults(FanoutArgs a, FaultArgs f, ExactArgs xa) {
    fanout_count_body<true, true>(a, f, xa);
}

// Exact-k fanout, the pass in front of the count pass: bound[u] = q(u, T) and the out side of every node, one
// lane per row (the head of this file).  SLOTS: the LDS slots per lane, 8 or 32 -- the host picks the
// smaller one that holds the largest k of a selecting node (16 KiB or 64 KiB a block).
template <uint32_t SLOTS>
__global__ __launch_bounds__(256) void k_fanout_kth(FanoutArgs a, ExactArgs xa) {
    __shared__ uint64_t s_keep[SLOTS][256];
    const uint32_t tid = threadIdx.x;
    unsigned long long tout = 0ull;
    for (uint64_t u = (uint64_t)blockIdx.x * 256u + tid; u < a.n; u += (uint64_t)gridDim.x * 256u) {
        const uint32_t k = xa.kx[u];
        uint32_t oc = xa.xout[u];
        uint64_t bd = kFanoutExactAll;
        if (k != 0u && k <= SLOTS) {  // (k <= SLOTS always: the host's choice; the bound on the LDS index)
            FanoutExactTop s = {0ull, 0u, 0u, 0u};
            for (int64_t j = a.rowptr[u], je = a.rowptr[u + 1u]; j < je; j++) {
                const uint32_t v = (uint32_t)a.col[j], mo = (uint32_t)a.emult[j] >> 4;
                for (uint32_t c = 0; c < mo; c++)
                    fanout_exact_push(s, &s_keep[0][tid], 256u, k, fanout_exact_draw(a.seed, (uint32_t)u, v, c, a.tick));
            }
            bd = s.mx;
            oc = s.have + s.ties;
        }
        xa.bound[u] = bd;
        const uint32_t r = a.recv[u], g = a.gen[u];
        const uint32_t d = (r - a.recv_prev[u]) + (g - a.gen_prev[u]);
        if (d && oc) a.sent_f[u] += (unsigned long long)oc * d;
        a.recv_prev[u] = r;
        a.gen_prev[u] = g;
        tout += oc;
    }
    for (int off = 32; off > 0; off >>= 1) tout += __shfl_xor(tout, off, 64);
    if ((tid & 63u) == 0u && tout) atomicAdd(a.stat + (blockIdx.x & (kFanoutStatReplicas - 1u)) * kFanoutStatLine + 1, tout);
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
