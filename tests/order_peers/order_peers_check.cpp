// Stand-alone check of gossip::order_peers (csrc/internal.h), built with -fsanitize=address,undefined
// by tests/test_order_peers.py: every row stays a permutation of itself, the order inside a row is
// (sockets descending, id ascending), and empty rows, n = 0 and any thread count work.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "internal.h"

static int fails = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            fails++;                                               \
        }                                                          \
    } while (0)

static void check_graph(uint32_t n, const std::vector<int64_t>& rp, const std::vector<int32_t>& col0,
                        const std::vector<uint32_t>& sockets, int threads) {
    std::vector<int32_t> col = col0;
    gossip::order_peers(n, rp.data(), col.data(), sockets.data(), threads);
    CHECK(col.size() == col0.size());
    for (uint32_t v = 0; v < n; v++) {
        std::vector<int32_t> x(col0.begin() + rp[v], col0.begin() + rp[v + 1]);
        std::vector<int32_t> y(col.begin() + rp[v], col.begin() + rp[v + 1]);
        for (size_t k = 1; k < y.size(); k++) {
            const uint32_t sa = sockets[y[k - 1]], sb = sockets[y[k]];
            CHECK(sa > sb || (sa == sb && y[k - 1] <= y[k]));
        }
        std::sort(x.begin(), x.end());
        std::sort(y.begin(), y.end());
        CHECK(x == y);
    }
    // a second pass over sorted rows changes nothing
    std::vector<int32_t> again = col;
    gossip::order_peers(n, rp.data(), again.data(), sockets.data(), threads);
    CHECK(again == col);
}

int main() {
    // n = 0: one row pointer, no entries, null column array
    {
        const int64_t rp0[1] = {0};
        gossip::order_peers(0, rp0, nullptr, nullptr, 4);
        gossip::order_peers(0, rp0, nullptr, nullptr, 1);
    }
    // a hand-made graph: rows with ties, an empty row, a row of one
    {
        // sockets (= row lengths): node 0: 3, 1: 2, 2: 2, 3: 0, 4: 1, 5: 2
        const std::vector<int64_t> rp = {0, 3, 5, 7, 7, 8, 10};
        const std::vector<int32_t> col = {4, 2, 1, /**/ 5, 0, /**/ 5, 0, /**/ /**/ 0, /**/ 2, 1};
        std::vector<uint32_t> so(6);
        for (int v = 0; v < 6; v++) so[v] = (uint32_t)(rp[v + 1] - rp[v]);
        std::vector<int32_t> c = col;
        gossip::order_peers(6, rp.data(), c.data(), so.data(), 3);
        const std::vector<int32_t> want = {1, 2, 4, /**/ 0, 5, /**/ 0, 5, /**/ /**/ 0, /**/ 1, 2};
        CHECK(c == want);
        for (int th : {1, 2, 16, 64}) check_graph(6, rp, col, so, th);
    }
    // random graphs (symmetric or not does not matter here): rows of 0 .. 70 entries, shuffled,
    // duplicates allowed, node counts around the thread split
    std::mt19937 rng(12345);
    for (uint32_t n : {1u, 2u, 15u, 16u, 17u, 257u, 1000u}) {
        std::vector<int64_t> rp(n + 1, 0);
        std::vector<int32_t> col;
        for (uint32_t v = 0; v < n; v++) {
            const uint32_t d = rng() % 4 == 0 ? 0u : rng() % 71u;
            for (uint32_t k = 0; k < d; k++) col.push_back((int32_t)(rng() % n));
            rp[v + 1] = (int64_t)col.size();
        }
        std::vector<uint32_t> so(n);
        for (uint32_t v = 0; v < n; v++) so[v] = (uint32_t)(rp[v + 1] - rp[v]);
        for (int th : {1, 4, 16}) check_graph(n, rp, col, so, th);
        // sockets unrelated to the row lengths (many ties)
        for (uint32_t v = 0; v < n; v++) so[v] = rng() % 3u;
        check_graph(n, rp, col, so, 16);
    }
    if (fails) {
        std::printf("%d checks FAILED\n", fails);
        return 1;
    }
    std::printf("order_peers: checks passed\n");
    return 0;
}
