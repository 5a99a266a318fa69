// Stand-alone check of the row message's rules (csrc/row_msg.h), built with
// -fsanitize=address,undefined by tests/test_row_msg.py: the layout against prefix sizes written out
// here (not a second copy of the rule), the checked inverse of the message length, the chunk
// geometry of every rank extent up to 5000 rows in 1 .. 16 chunks, and the broadcast capacities.
#include <cstdint>
#include <cstdio>

#include "row_msg.h"

static int fails = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            fails++;                                               \
        }                                                          \
    } while (0)

using gossip::RowChunk;
using gossip::RowMsgLayout;
using gossip::row_msg_chunk;
using gossip::row_msg_layout;
using gossip::row_msg_next_cap;
using gossip::row_msg_worst_rows;

int main() {
    // layout: prefix words (header + occupancy + offsets + liveness) of three messages
    {
        CHECK(row_msg_layout(0, 1, 2).rows == 4);
        CHECK(row_msg_layout(76, 1, 0).rows == 116);
        CHECK(row_msg_layout(512, 2, 64).rows == 1346);
        const RowMsgLayout L = row_msg_layout(512, 2, 64);
        CHECK(L.nz == 1 && L.off == 1025 && L.live == 1282 && L.rows == 1346);
        // k + 1 uint32 offsets in (k + 2) / 2 words: an odd k and the even k + 1 differ by one word
        CHECK(row_msg_layout(75, 1, 0).live - row_msg_layout(75, 1, 0).off == 38);
        CHECK(row_msg_layout(76, 1, 0).live - row_msg_layout(76, 1, 0).off == 39);
        CHECK(row_msg_layout(77, 1, 0).live - row_msg_layout(77, 1, 0).off == 39);
        const uint32_t ntws[3] = {1, 2, 3}, wlives[3] = {0, 2, 64};
        for (uint64_t k = 0; k <= 2048; k++)
            for (uint32_t ntw : ntws)
                for (uint32_t wl : wlives) {
                    const RowMsgLayout M = row_msg_layout(k, ntw, wl);
                    // (a message of no nodes has no occupancy words: nz == off at k = 0 only)
                    CHECK(M.nz == 1 && (k ? M.nz < M.off : M.nz == M.off));
                    CHECK(M.off < M.live && M.live <= M.rows);
                    CHECK(M.off - M.nz == k * ntw && 2 * (M.live - M.off) >= k + 1 && M.rows - M.live == wl);
                    CHECK((k & 1) || row_msg_layout(k + 1, ntw, wl).live - row_msg_layout(k + 1, ntw, wl).off ==
                                         M.live - M.off);
                }
    }
    // the length of a message and its checked inverse
    {
        const RowMsgLayout Ls[3] = {row_msg_layout(0, 1, 2), row_msg_layout(76, 1, 0), row_msg_layout(512, 2, 64)};
        for (const RowMsgLayout& L : Ls) {
            for (uint64_t r = 0; r <= 300; r++) {
                uint64_t n = ~0ull;
                CHECK(L.total_words(r) == L.rows + 16 * r);
                CHECK(L.nrows(L.total_words(r), &n) && n == r);
                for (uint64_t x = 1; x < 16; x++) CHECK(!L.nrows(L.total_words(r) + x, &n));
            }
            uint64_t n = 7;
            for (uint64_t w = 0; w < L.rows; w++) CHECK(!L.nrows(w, &n));
            CHECK(n == 7);  // (a refusal writes nothing)
        }
    }
    // chunks: disjoint, in order, their union the rank's rows, boundaries on 512-row granules
    {
        const uint32_t hw = 48;
        const uint64_t as[2] = {0, 1536};
        for (uint64_t a : as)
            for (uint64_t ext = 0; ext <= 5000; ext++) {
                const uint64_t b = a + ext;
                for (uint32_t nch = 1; nch <= 16; nch++) {
                    uint64_t at = a;
                    for (uint32_t c = 0; c < nch; c++) {
                        const RowChunk ch = row_msg_chunk(a, b, nch, c, hw);
                        CHECK(ch.lo == at && ch.hi >= ch.lo && ch.hi <= b);
                        CHECK(ch.hi == b || (ch.hi - a) % 512 == 0);
                        CHECK(ch.wlive == (c + 1 >= nch ? hw : 0u));
                        at = ch.hi;
                    }
                    CHECK(at == b);
                    const RowChunk whole = row_msg_chunk(a, b, nch, gossip::kWholeRows, hw);
                    CHECK(whole.lo == a && whole.hi == b && whole.wlive == hw);
                }
            }
        RowChunk ch = row_msg_chunk(0, 1024, 2, 0, hw);
        CHECK(ch.lo == 0 && ch.hi == 512 && ch.wlive == 0);
        ch = row_msg_chunk(0, 1024, 2, 1, hw);
        CHECK(ch.lo == 512 && ch.hi == 1024 && ch.wlive == hw);
        ch = row_msg_chunk(1024, 1100, 2, 0, hw);  // 76 rows: all in chunk 0 ...
        CHECK(ch.lo == 1024 && ch.hi == 1100 && ch.wlive == 0);
        ch = row_msg_chunk(1024, 1100, 2, 1, hw);  // ... and an empty last chunk with the liveness
        CHECK(ch.lo == 1100 && ch.hi == 1100 && ch.wlive == hw);
        for (uint32_t c = 0; c < 16; c++) {  // 476 rows in 16 chunks
            ch = row_msg_chunk(1024, 1500, 16, c, hw);
            CHECK(ch.lo == (c ? 1500u : 1024u) && ch.hi == 1500 && ch.wlive == (c == 15 ? hw : 0u));
        }
    }
    // capacities: worst case = every tile row; growth to 1.25x + 16, capped; kept while enough
    {
        CHECK(row_msg_worst_rows(512, 32) == 1024 && row_msg_worst_rows(76, 16) == 76 && row_msg_worst_rows(0, 64) == 0);
        CHECK(row_msg_next_cap(100, 0, 512, 32) == 141);
        CHECK(row_msg_next_cap(1000, 0, 512, 32) == 1024);
        CHECK(row_msg_next_cap(100, 141, 512, 32) == 141 && row_msg_next_cap(141, 141, 512, 32) == 141);
        CHECK(row_msg_next_cap(0, 0, 512, 32) == 0);
        const uint64_t ks[3] = {76, 512, 1024};
        const uint32_t hws[3] = {16, 32, 1216};
        for (uint64_t k : ks)
            for (uint32_t hw : hws) {
                const uint64_t worst = row_msg_worst_rows(k, hw);
                for (uint64_t cap = 0; cap <= worst; cap += 1 + worst / 37)
                    for (uint64_t tot = 0; tot <= worst; tot += 1 + worst / 53) {
                        const uint64_t next = row_msg_next_cap(tot, cap, k, hw);
                        CHECK(next >= tot && next <= worst && next >= cap);
                        CHECK(tot > cap || next == cap);
                    }
                CHECK(row_msg_next_cap(worst, 0, k, hw) == worst);
            }
    }
    if (fails) {
        std::printf("%d checks FAILED\n", fails);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
