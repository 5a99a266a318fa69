// row_msg.h -- the row partition's frontier message as host-only rules (no HIP, no device code):
// its layout, the rows of a (rank, chunk), and the row capacity of a broadcast.  The rules live here
// alone: the packer, the unpacker and the three transports (engine.hip: RCCL, lockstep,
// host-staged) all read them, none derives them again.
//
// A rank's message for tick t and row chunk c: its rows [lo, hi) of F_next (the chunk, or all its
// rows), restricted to OCCUPIED 16-word tile rows (the nz bits; unoccupied rows hold stale words no
// reader loads), plus -- in its last chunk only -- its partial liveness.  In uint64 words, with
// k = hi - lo nodes:
//   [0]                       the row count N: the last element of the exclusive scan of the
//                             nodes' occupied-row counts, copied on the device (k_msg_header)
//   [nz,   nz + k * ntw)      occupancy (nz) words of nodes lo .. hi-1
//   [off,  off + (k + 2) / 2) k + 1 uint32 row offsets: node lo+i's rows start at offset[i]
//   [live, live + wlive)      liveness words of the rank's rows (last chunk / whole rows, else none)
//   [rows, rows + 16 N)       the rows, node by node, tile by tile
// Everything before the rows is the PREFIX: its size follows from (rank, chunk) alone, so a
// receiver places every part without reading the message, a broadcast can carry the prefix and a
// row capacity agreed beforehand, and N follows from a whole message's length.
#pragma once

#include <stdint.h>

#include <algorithm>

namespace gossip {

constexpr uint32_t kRowMsgRowWords = 16;    // one tile row (the engine's kTileWords)
constexpr uint64_t kRowGranule = 512;       // chunk boundaries: the dense tile and the row-partition block
constexpr uint32_t kWholeRows = 0xffffffffu;  // chunk index: one message of all of a rank's rows

struct RowMsgLayout {
    uint64_t nz, off, live, rows;  // word offsets of the parts; rows = prefix words
    uint64_t total_words(uint64_t nrows) const { return rows + (uint64_t)kRowMsgRowWords * nrows; }
    // the row count of a whole message of `words` words; false: no message of this layout is so long
    bool nrows(uint64_t words, uint64_t* n) const {
        if (words < rows || (words - rows) % kRowMsgRowWords) return false;
        *n = (words - rows) / kRowMsgRowWords;
        return true;
    }
};
inline RowMsgLayout row_msg_layout(uint64_t k, uint32_t ntw, uint32_t wlive) {
    RowMsgLayout L;
    L.nz = 1;
    L.off = L.nz + k * ntw;
    L.live = L.off + (k + 2) / 2;
    L.rows = L.live + wlive;
    return L;
}

// Chunk c of `nchunks` of a rank that owns rows [a, b): whole granules, the last chunks possibly
// empty; kWholeRows = all of them.  The rank's hw liveness words ride in its last chunk, empty or
// not (and in a whole-rows message).
struct RowChunk {
    uint64_t lo, hi;
    uint32_t wlive;
};
inline RowChunk row_msg_chunk(uint64_t a, uint64_t b, uint32_t nchunks, uint32_t c, uint32_t hw) {
    if (c == kWholeRows || nchunks <= 1) return RowChunk{a, b, hw};
    const uint64_t per = ((b - a + nchunks - 1) / nchunks + kRowGranule - 1) / kRowGranule * kRowGranule;
    const uint64_t lo = std::min<uint64_t>(b, a + (uint64_t)c * per);
    return RowChunk{lo, std::min<uint64_t>(b, lo + per), c + 1 >= nchunks ? hw : 0u};
}

// Most rows a message of k nodes can hold: every tile row of hw live words.
inline uint64_t row_msg_worst_rows(uint64_t k, uint32_t hw) { return k * (hw / kRowMsgRowWords); }

// Row capacity of a (rank, chunk)'s next broadcast after a tick that packed `tot` rows: kept while
// it sufficed, else 1.25x the count seen, at most the worst case.
inline uint64_t row_msg_next_cap(uint64_t tot, uint64_t cap, uint64_t k, uint32_t hw) {
    return tot <= cap ? cap : std::min<uint64_t>(tot + tot / 4 + 16, row_msg_worst_rows(k, hw));
}

}  // namespace gossip
