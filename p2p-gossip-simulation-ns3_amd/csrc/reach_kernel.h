// reach_kernel.h -- reach profiles (GOSSIP_F_REACH): per share column, the number of nodes whose
// first contact with the share happened this tick = the column sums of the tick's new-bit matrix
// over the engine's own rows [v0, v1) and the allocated tiles of the window.  Launched from
// tick_step_b after the tick's births and exchange; the host folds the counts into (event, hop)
// bins (engine.hip reach_fold_slot).
//
// Where a tick's new bits live is decode_trace's rule (engine.hip), case by case, per tile mode:
//   RM_NZ     the tile's dense row of a node is valid only behind its occupancy bit (stale
//             otherwise): the 128-B line is skipped
//   RM_WS     write-sparse young tile: the bits are in the node's slot entries (k_reach_slots);
//             only an overflowed node (header 0xffff) holds them in its dense row, read here
//             without an occupancy bit
//   RM_FOLDF  folded row (seen | new) of a tile that was TM_SEENF this tick: masked with the
//             node's row in the other frontier buffer
//   RM_FOLDS  folded row of a tile that was not: masked with the node's seen row
// DENSE mode, hop batches, link timing and keep masks leave post-keep new bits in the same rows.
//
// Counting (k_reach): a block takes one tile and a range of rows; lane l owns word l & 15 of the
// tile and rows l >> 4 (+ 4 per wave, + 16 per step), so one wave load is four whole 128-B lines.
// The lane adds its words into kReachPlanes carry-save bit planes (plane k = bit k of 64 vertical
// counters): no per-bit work per row.  The planes are flushed into per-column u32 counts in LDS
// after at most `flush` rows (<= kReachCap, the planes' capacity) and at the end of the block's
// rows; one global atomic per non-zero column then adds the block's counts to the tick's array.
//
// The plane functions are host/device so that tests/reach_planes checks them on the CPU.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define REACH_HD __host__ __device__ inline
#else
#define REACH_HD inline
#endif

namespace gossip {

constexpr uint32_t kReachPlanes = 8;                        // binary digits per vertical counter
constexpr uint32_t kReachCap = (1u << kReachPlanes) - 1u;   // rows a lane may add between flushes
constexpr uint32_t kReachRowsPerStep = 16;                  // rows a block's four waves load per step
constexpr uint32_t kReachInflight = 8;                      // rows a lane loads before it waits (multiple of 4)
constexpr uint32_t kReachSlotLdsTiles = 8;                  // k_reach_slots: write-sparse tiles whose
                                                            // counters (4 KiB each) are kept in LDS

// tile modes (ReachArgs::tiles entries: tile | mode << 24)
enum : uint32_t { RM_NZ = 1u, RM_WS = 2u, RM_FOLDF = 4u, RM_FOLDS = 8u };

// planes += x (one row): ripple carry through every plane
REACH_HD void reach_plane_add(uint64_t* p, uint64_t x) {
#pragma unroll
    for (uint32_t k = 0; k < kReachPlanes; k++) {
        const uint64_t c = p[k] & x;
        p[k] ^= x;
        x = c;
    }
}

// planes += a + b + c + d (four rows): three carry-save adders, then one ripple from plane 2
REACH_HD void reach_plane_add4(uint64_t* p, uint64_t a, uint64_t b, uint64_t c, uint64_t d) {
    const uint64_t s1 = p[0] ^ a ^ b, t1 = (p[0] & a) | ((p[0] ^ a) & b);
    const uint64_t s2 = s1 ^ c ^ d, t2 = (s1 & c) | ((s1 ^ c) & d);
    p[0] = s2;
    const uint64_t s3 = p[1] ^ t1 ^ t2;
    uint64_t x = (p[1] & t1) | ((p[1] ^ t1) & t2);
    p[1] = s3;
#pragma unroll
    for (uint32_t k = 2; k < kReachPlanes; k++) {
        const uint64_t cy = p[k] & x;
        p[k] ^= x;
        x = cy;
    }
}

// the counter of column b
REACH_HD uint32_t reach_plane_count(const uint64_t* p, uint32_t b) {
    uint32_t c = 0;
#pragma unroll
    for (uint32_t k = 0; k < kReachPlanes; k++) c |= (uint32_t)((p[k] >> b) & 1ull) << k;
    return c;
}

// add(b, count) for every non-zero column counter, then planes = 0
template <class Add>
REACH_HD void reach_plane_flush(uint64_t* p, Add add) {
    uint64_t any = 0ull;
#pragma unroll
    for (uint32_t k = 0; k < kReachPlanes; k++) any |= p[k];
    for (uint64_t m = any; m; m &= m - 1ull) {
        const uint32_t b = (uint32_t)__builtin_ctzll(m);
        add(b, reach_plane_count(p, b));
    }
#pragma unroll
    for (uint32_t k = 0; k < kReachPlanes; k++) p[k] = 0ull;
}

// One step of a lane: four more rows into the planes, flushing through add(b, count) whenever the
// lane has added `cap` rows (1 .. kReachCap) since its last flush.  added: rows since that flush.
template <class Add>
REACH_HD void reach_lane_step(uint64_t* p, uint32_t& added, uint32_t cap, uint64_t x0, uint64_t x1, uint64_t x2,
                              uint64_t x3, Add add) {
    if (added + 4u <= cap) {
        reach_plane_add4(p, x0, x1, x2, x3);
        added += 4u;
        return;
    }
    const uint64_t xs[4] = {x0, x1, x2, x3};
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        if (added >= cap) {
            reach_plane_flush(p, add);
            added = 0;
        }
        reach_plane_add(p, xs[k]);
        added++;
    }
}

#if defined(__HIPCC__)

struct ReachArgs {
    const uint64_t* F;             // the frontier buffer the tick wrote (F_next)
    const uint64_t* Fprev;         // the other one (the tick read it): RM_FOLDF mask
    const uint64_t* seen;          // row v at seen + v * stride: RM_FOLDS mask
    const unsigned long long* nz;  // F's occupancy words (n x ntw), or nullptr
    const uint16_t* slot;          // F's slots (n x 128 u16), or nullptr
    const uint32_t* tiles;         // tile | mode << 24, one per block column
    uint32_t stride, ntw;
    uint32_t v0, v1;               // own rows
    uint32_t rows_per_block;       // multiple of kReachInflight * kReachRowsPerStep
    uint32_t flush;                // rows a lane adds between flushes, 1 .. kReachCap
    uint32_t* cnt;                 // per column of the window: this tick's counts
    unsigned long long* bytes;     // bytes loaded
};

// grid (tiles, row blocks), 256 threads
__global__ __launch_bounds__(256) void k_reach(ReachArgs a) {
    __shared__ uint32_t s_cnt[1024];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, q = lane & 15u, sub = lane >> 4;
    const uint32_t te = a.tiles[blockIdx.x];
    const uint32_t tl = te & 0xffffffu, mode = te >> 24;
    for (uint32_t c = threadIdx.x; c < 1024u; c += 256u) s_cnt[c] = 0u;
    __syncthreads();
    const uint64_t r_begin = (uint64_t)a.v0 + (uint64_t)blockIdx.y * a.rows_per_block;
    const uint64_t r_end = r_begin + a.rows_per_block < a.v1 ? r_begin + a.rows_per_block : (uint64_t)a.v1;
    const uint32_t tw = tl >> 6;
    const unsigned long long tbit = 1ull << (tl & 63u);
    const uint64_t woff = (uint64_t)tl * 16u + q;
    uint32_t nbytes = 0;
    // the fold mask's source, if the tile is folded (block-uniform)
    const uint64_t* mask = (mode & RM_FOLDF) ? a.Fprev : (mode & RM_FOLDS) ? a.seen : nullptr;
    uint64_t p[kReachPlanes];
#pragma unroll
    for (uint32_t k = 0; k < kReachPlanes; k++) p[k] = 0ull;
    auto add = [&](uint32_t b, uint32_t c) { atomicAdd(&s_cnt[q * 64u + b], c); };
    uint32_t added = 0;  // rows since the last flush (block-uniform: rows past r_end count as zeros)
    // A pass of the loop takes kReachInflight rows per lane in three stages, each stage's loads
    // issued together before any of them is waited for: the rows' gates (occupancy word or slot
    // header), then the gated row words and their mask words, then the adds.  A wave so keeps
    // kReachInflight (x 2, folded) 512-B loads in flight, not one behind each gate.
    for (uint64_t base = r_begin; base < r_end; base += (uint64_t)kReachInflight * kReachRowsPerStep) {
        uint64_t r[kReachInflight], x[kReachInflight], m[kReachInflight];
        bool ok[kReachInflight];
#pragma unroll
        for (uint32_t k = 0; k < kReachInflight; k++) {
            r[k] = base + wv * 4u + sub + (uint64_t)k * kReachRowsPerStep;
            ok[k] = r[k] < r_end;
        }
        if (mode & RM_NZ) {
            unsigned long long g[kReachInflight];
#pragma unroll
            for (uint32_t k = 0; k < kReachInflight; k++) g[k] = ok[k] ? a.nz[r[k] * a.ntw + tw] : 0ull;
#pragma unroll
            for (uint32_t k = 0; k < kReachInflight; k++) {
                nbytes += (ok[k] && q == 0u) ? 8u : 0u;
                ok[k] = (g[k] & tbit) != 0ull;
            }
        } else if (mode & RM_WS) {
            uint32_t h[kReachInflight];
#pragma unroll
            for (uint32_t k = 0; k < kReachInflight; k++)  // (the header's 4-B word: a slot is 256-B aligned;
                                                            //  a row past the end reads row r_begin's: no branch)
                h[k] = *reinterpret_cast<const uint32_t*>(a.slot + (ok[k] ? r[k] : r_begin) * 128u);
#pragma unroll
            for (uint32_t k = 0; k < kReachInflight; k++) {
                nbytes += (ok[k] && q == 0u) ? 4u : 0u;
                ok[k] = ok[k] && (h[k] & 0xffffu) == 0xffffu;
            }
        }
        if (mask) {  // (block-uniform: a row's word and its mask word leave together)
#pragma unroll
            for (uint32_t k = 0; k < kReachInflight; k++) {
                const uint64_t at = r[k] * a.stride + woff;
                x[k] = ok[k] ? a.F[at] : 0ull;
                m[k] = ok[k] ? mask[at] : 0ull;
            }
        } else {
#pragma unroll
            for (uint32_t k = 0; k < kReachInflight; k++) {
                x[k] = ok[k] ? a.F[r[k] * a.stride + woff] : 0ull;
                m[k] = 0ull;
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < kReachInflight; k++) {
            nbytes += ok[k] ? (mask ? 16u : 8u) : 0u;
            x[k] &= ~m[k];
        }
#pragma unroll
        for (uint32_t k = 0; k < kReachInflight; k += 4)
            reach_lane_step(p, added, a.flush, x[k], x[k + 1], x[k + 2], x[k + 3], add);
    }
    reach_plane_flush(p, add);
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < 1024u; c += 256u) {
        const uint32_t x = s_cnt[c];
        if (x) atomicAdd(&a.cnt[(uint64_t)tl * 1024u + c], x);
    }
    for (int off = 32; off > 0; off >>= 1) nbytes += __shfl_xor(nbytes, off, 64);
    if (lane == 0 && nbytes) atomicAdd(a.bytes, (unsigned long long)nbytes);
}

struct ReachSlotArgs {
    const uint16_t* slot;       // F_next's slots
    const uint32_t* wt;         // write-sparse index -> tile
    uint32_t nwt;
    uint32_t lds_lo;            // write-sparse indices [lds_lo, nwt) are counted in LDS
    uint32_t v0, v1;
    uint32_t* cnt;
    unsigned long long* bytes;
};

// The write-sparse tiles' slot entries, one wave per node: entry e = widx << 10 | word << 6 | bit.
// The counters of the tiles [lds_lo, nwt) -- at most kReachSlotLdsTiles, the LAST indices: the
// host lists write-sparse tiles youngest first, and the oldest hold nearly all entries (a share's
// frontier grows by the degree every hop) -- are block-local in LDS, one global atomic per non-zero
// column at the end; an entry of a tile below lds_lo (the counter set did not fit) is one global
// atomic.  Dynamic LDS: (nwt - lds_lo) x 4 KiB.
__global__ __launch_bounds__(256) void k_reach_slots(ReachSlotArgs a) {
    extern __shared__ uint32_t s_c[];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t nlds = (a.nwt - a.lds_lo) * 1024u, e_lo = a.lds_lo << 10;
    for (uint32_t c = threadIdx.x; c < nlds; c += 256u) s_c[c] = 0u;
    __syncthreads();
    uint32_t nbytes = 0;
    for (uint64_t v = (uint64_t)a.v0 + (uint64_t)blockIdx.x * 4u + wv; v < a.v1; v += (uint64_t)gridDim.x * 4u) {
        const uint32_t* sl = reinterpret_cast<const uint32_t*>(a.slot + v * 128u);
        uint32_t x = lane < 32u ? sl[lane] : 0xffffffffu;
        const uint32_t hdr = __shfl(x, 0, 64) & 0xffffu;
        nbytes += lane == 0u ? 128u : 0u;
        if (hdr == 0xffffu) continue;  // overflowed: its dense rows (k_reach, RM_WS)
        if (hdr > 63u) {               // the second line
            if (lane >= 32u) x = sl[lane];
            nbytes += lane == 0u ? 128u : 0u;
        }
#pragma unroll
        for (uint32_t h = 0; h < 2; h++) {
            const uint32_t k = 2u * lane + h, e = h ? x >> 16 : x & 0xffffu;
            if (k == 0u || k > hdr || e == 0xffffu || (e >> 10) >= a.nwt) continue;  // header, unused, tombstone
            if (e >= e_lo)
                atomicAdd(&s_c[e - e_lo], 1u);  // (e = widx * 1024 + column in the tile)
            else
                atomicAdd(&a.cnt[(uint64_t)a.wt[e >> 10] * 1024u + (e & 1023u)], 1u);
        }
    }
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < nlds; c += 256u) {
        const uint32_t x = s_c[c];
        if (x) atomicAdd(&a.cnt[(uint64_t)a.wt[a.lds_lo + (c >> 10)] * 1024u + (c & 1023u)], x);
    }
    for (int off = 32; off > 0; off >>= 1) nbytes += __shfl_xor(nbytes, off, 64);
    if (lane == 0 && nbytes) atomicAdd(a.bytes, (unsigned long long)nbytes);
}

#endif  // __HIPCC__

}  // namespace gossip
