// rounds_kernel.h -- multi-round push (gossip.h, gossip_engine_set_rounds): a node that first contacts a
// share in tick T makes Sends of it in ticks T .. T + r - 1.  The pull kernels and the six fanout kernels
// do not change: k_rounds, once per tick between the reach pass and the fanout passes, turns the frontier
// rows the tick wrote ("new bits of tick t") into the node's send set of the tick and keeps the remaining
// rounds of every (node, share bit).
//
// Counters.  The remaining rounds of (node v, column c) are a down-counter in [0, r - 1], bit-sliced over
// P = bit_length(r - 1) <= 4 planes, each with the shape of a frontier buffer (n x stride words): plane k
// holds bit k of the counters of a word's 64 columns.  The planes always hold the truth (zero where nothing
// is pending); an occupancy bit per (node, tile) -- pnz, the shape of the frontier's occupancy words -- says
// that some plane word of the node's tile row is non-zero, so a row with no new bits and no pending counter
// costs its two 8-B gate words per 64 tiles and no row traffic.
//
// Per (node v, tile) with a gate bit, per word (new = the tick's new bits, 0 behind a clear occupancy bit:
// such a row is stale):
//     old    = nonzero(planes) & keep & ~down(v, tick)         re-sends of this tick
//     S      = new | old                                       (disjoint: an old bit is a seen bit)
//     planes = decrement where non-zero; r - 1 where new; 0 where the column is not kept
//     F_next word <- S (the whole 128-B row when the occupancy bit was clear), occupancy bit |= (S != 0 in the
//     row), liveness word |= S | nonzero(planes), send_cum[v] += popcount(S), pnz bit = nonzero(planes) in the row
// keep is the tick's keep mask of the word (WordCtl::keep: the columns whose arrivals in this tick count,
// i.e. the columns that are alive in it); down is fanout_kernel.h's outage_down.  The decrement happens for
// a down node too: its rounds elapse.
// Liveness carries the pending counters as well as S, so that a column with a pending re-send at a node
// that is down stays live: live columns then only die (what the saturation bits of k_pull rely on), and a
// word retires only when every counter in it is 0 (retire_from reads these words), so a re-used word starts
// with clean planes.
//
// Access shape.  A block takes one occupancy word (64 tiles) at a time and strides over groups of 16 rows;
// a wave takes 4 rows, 16 lanes each: lane q of a row owns word q of a tile row, so a wave access is four
// whole 128-B lines.  The 16 lanes of a row walk the set bits of (occupancy | pnz) together.  Liveness is
// ORed into the block's LDS copy of the occupancy word's 1,024 words and leaves with one global atomic per
// non-zero word per block; a node's popcount is summed over its tiles and its 16 lanes before one atomic.
//
// The plane functions are host/device so that tests/rounds_planes checks them on the CPU.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include "fanout_kernel.h"  // outage_down
#define ROUNDS_HD __host__ __device__ inline
#else
#define ROUNDS_HD inline
#endif

namespace gossip {

constexpr uint32_t kRoundsMax = 16;       // largest r
constexpr uint32_t kRoundsMaxPlanes = 4;  // bit_length(kRoundsMax - 1)

// planes of r rounds: bit_length(r - 1); 0 at r = 1 (no counter: the feature is off)
ROUNDS_HD uint32_t rounds_planes(uint32_t r) {
    uint32_t p = 0;
    for (uint32_t x = r > 0 ? r - 1u : 0u; x; x >>= 1) p++;
    return p;
}

// columns whose counter is not 0
ROUNDS_HD uint64_t rounds_plane_nonzero(const uint64_t* p, uint32_t np) {
    uint64_t m = 0ull;
#pragma unroll
    for (uint32_t k = 0; k < kRoundsMaxPlanes; k++)
        if (k < np) m |= p[k];
    return m;
}

// counter = value (< 2^np) in the columns of mask
ROUNDS_HD void rounds_plane_set(uint64_t* p, uint32_t np, uint64_t mask, uint32_t value) {
#pragma unroll
    for (uint32_t k = 0; k < kRoundsMaxPlanes; k++)
        if (k < np) p[k] = (p[k] & ~mask) | (((value >> k) & 1u) ? mask : 0ull);
}

// counter -= 1 where it is not 0: a borrow ripples up from plane 0 through the planes that hold a 0
ROUNDS_HD void rounds_plane_dec(uint64_t* p, uint32_t np) {
    uint64_t borrow = rounds_plane_nonzero(p, np);
#pragma unroll
    for (uint32_t k = 0; k < kRoundsMaxPlanes; k++)
        if (k < np) {
            const uint64_t x = p[k];
            p[k] = x ^ borrow;
            borrow &= ~x;
        }
}

// the counter of column b
ROUNDS_HD uint32_t rounds_plane_count(const uint64_t* p, uint32_t np, uint32_t b) {
    uint32_t c = 0;
#pragma unroll
    for (uint32_t k = 0; k < kRoundsMaxPlanes; k++)
        if (k < np) c |= (uint32_t)((p[k] >> b) & 1ull) << k;
    return c;
}

// One word's step of a tick: the planes' update, and the send set returned.  fresh: the tick's new bits;
// keep: the columns alive in the tick; down: the node is down in it.  *old = the re-sent bits.
ROUNDS_HD uint64_t rounds_word_step(uint64_t* p, uint32_t np, uint32_t r, uint64_t fresh, uint64_t keep, bool down, uint64_t* old) {
    const uint64_t o = down ? 0ull : rounds_plane_nonzero(p, np) & keep & ~fresh;
    rounds_plane_dec(p, np);
    rounds_plane_set(p, np, fresh, r - 1u);
    rounds_plane_set(p, np, ~keep, 0u);
    *old = o;
    return fresh | o;
}

#if defined(__HIPCC__)

// [0] re-sent bits, [1] (row, tile) pairs visited, [2] bytes moved
constexpr uint32_t kRoundsStats = 3;

struct RoundsArgs {
    uint64_t* F;                    // the frontier buffer the tick wrote (F_next): new bits in, send sets out
    unsigned long long* nz;         // its occupancy words (n x ntw)
    uint64_t* plane[kRoundsMaxPlanes];
    unsigned long long* pnz;        // the planes' occupancy words (n x ntw)
    const uint64_t* keep;           // the tick's WordCtl array: keep at keep[w * keep_stride] (u64 units)
    uint32_t keep_stride;
    unsigned long long* live;       // the tick's liveness words
    uint32_t* send_cum;             // per node: the sizes of its send sets, summed over ticks
    const uint32_t* out_off;        // outages (nullptr: none): fanout_kernel.h outage_down
    const uint32_t* out_from;
    const uint32_t* out_to;
    unsigned long long* stat;       // kRoundsStats words
    uint32_t stride, ntw, hw;       // words per row, occupancy words per row, allocated words (tiles < hw / 16)
    uint32_t v0, v1;                // own rows
    uint32_t r, np;
    uint32_t tick;
};

// grid: any number of 256-thread blocks (option rounds_grid); a block's step is 16 rows of one occupancy word
template <uint32_t NP>
__global__ __launch_bounds__(256) void k_rounds(RoundsArgs a) {
    __shared__ unsigned long long s_live[1024];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, q = lane & 15u, sub = lane >> 4;
    const uint64_t rows = (uint64_t)a.v1 - a.v0, ngrp = (rows + 15u) / 16u;
    const uint32_t ntiles = a.hw >> 4;
    unsigned long long resent = 0ull, visited = 0ull, nbytes = 0ull;
    const uint32_t ntw_live = (a.hw + 1023u) >> 10;  // (the occupancy words beyond hold no tile)
    for (uint32_t tw = 0; tw < ntw_live; tw++) {
        for (uint32_t i = threadIdx.x; i < 1024u; i += 256u) s_live[i] = 0ull;
        __syncthreads();
        for (uint64_t g = blockIdx.x; g < ngrp; g += gridDim.x) {
            const uint64_t v = (uint64_t)a.v0 + g * 16u + wv * 4u + sub;
            const bool ok = v < a.v1;
            const unsigned long long gn = ok ? a.nz[v * a.ntw + tw] : 0ull, gp = ok ? a.pnz[v * a.ntw + tw] : 0ull;
            nbytes += (ok && q == 0u) ? 16u : 0u;
            unsigned long long m = gn | gp;
            // (only a row with pending counters asks: a down node has no new bits)
            const bool dn = gp != 0ull && a.out_off != nullptr && outage_down(a.out_off, a.out_from, a.out_to, (uint32_t)v, (uint64_t)a.tick);
            unsigned long long nz_set = 0ull, pnz_set = 0ull, pnz_clr = 0ull;
            uint32_t pc = 0u;
            while (__ballot(m != 0ull)) {  // wave-uniform: a row that has run out of tiles idles with its lanes predicated off
                const bool act = m != 0ull;
                const uint32_t b = act ? (uint32_t)__builtin_ctzll(m) : 0u;
                m &= m - 1ull;
                const uint32_t tl = tw * 64u + b;
                const bool in = act && tl < ntiles;  // (the occupancy words name allocated tiles only: the bound on the index)
                const unsigned long long tbit = 1ull << b;
                const bool hn = in && (gn & tbit) != 0ull, hp = in && (gp & tbit) != 0ull;
                const uint32_t w = tl * 16u + q;
                const uint64_t at = v * a.stride + w;
                const uint64_t x = hn ? a.F[at] : 0ull;
                uint64_t p[kRoundsMaxPlanes] = {0ull, 0ull, 0ull, 0ull}, p0[kRoundsMaxPlanes] = {0ull, 0ull, 0ull, 0ull};
#pragma unroll
                for (uint32_t k = 0; k < NP; k++) p[k] = p0[k] = hp ? a.plane[k][at] : 0ull;
                const uint64_t keep = in ? a.keep[(uint64_t)w * a.keep_stride] : 0ull;
                uint64_t old;
                const uint64_t S = rounds_word_step(p, NP, a.r, x, keep, dn, &old);
#pragma unroll
                for (uint32_t k = 0; k < NP; k++)
                    if (p[k] != p0[k]) a.plane[k][at] = p[k];
                const uint64_t pend = rounds_plane_nonzero(p, NP);
                // the row's 16 lanes: any send bit, any pending counter
                const uint32_t sh = sub * 16u;
                const bool row_s = ((__ballot(S != 0ull) >> sh) & 0xffffull) != 0ull;
                const bool row_p = ((__ballot(pend != 0ull) >> sh) & 0xffffull) != 0ull;
                if (in) {
                    if (!hn && row_s) a.F[at] = S;  // a stale row: written whole
                    else if (S != x) a.F[at] = S;
                    if (!hn && row_s) nz_set |= tbit;
                    if (row_p && !hp) pnz_set |= tbit;
                    if (!row_p && hp) pnz_clr |= tbit;
                    if (S | pend) atomicOr(&s_live[b * 16u + q], (unsigned long long)(S | pend));
                    pc += (uint32_t)__popcll(S);
                    resent += (unsigned long long)__popcll(old);
                    visited += q == 0u ? 1u : 0u;
                    nbytes += (hn ? 8u : 0u) + (hp ? 8u * NP : 0u) + 8u + ((S != x || (!hn && row_s)) ? 8u : 0u);
#pragma unroll
                    for (uint32_t k = 0; k < NP; k++) nbytes += p[k] != p0[k] ? 8u : 0u;
                }
            }
            // the node's popcount over its 16 lanes, then one atomic (another block may hold its other occupancy words)
            pc += __shfl_xor(pc, 1, 64);
            pc += __shfl_xor(pc, 2, 64);
            pc += __shfl_xor(pc, 4, 64);
            pc += __shfl_xor(pc, 8, 64);
            if (ok && q == 0u) {
                if (pc) atomicAdd(&a.send_cum[v], pc);
                if (nz_set) atomicOr(&a.nz[v * a.ntw + tw], nz_set);
                if (pnz_set | pnz_clr) a.pnz[v * a.ntw + tw] = (gp | pnz_set) & ~pnz_clr;  // (this lane alone owns the word)
            }
        }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < 1024u; i += 256u) {
            const unsigned long long x = s_live[i];
            const uint32_t w = tw * 1024u + i;
            if (x && w < a.hw) atomicOr(&a.live[w], x);
        }
        __syncthreads();
    }
    for (int off = 32; off > 0; off >>= 1) {
        resent += __shfl_xor(resent, off, 64);
        visited += __shfl_xor(visited, off, 64);
        nbytes += __shfl_xor(nbytes, off, 64);
    }
    if (lane == 0) {
        if (resent) atomicAdd(a.stat, resent);
        if (visited) atomicAdd(a.stat + 1, visited);
        if (nbytes) atomicAdd(a.stat + 2, nbytes);
    }
}

#endif  // __HIPCC__

}  // namespace gossip
