// Stand-alone check of gossip::pull_shape (csrc/pull_plan.h), built with -fsanitize=address,undefined
// by tests/test_pull_plan.py: the launch shape of a k_pull window against a table written out here
// (not a second copy of the rule), the invariants every shape keeps, and TickPlan::reset.
#include <cstdint>
#include <cstdio>

#include "pull_plan.h"

static int fails = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            fails++;                                               \
        }                                                          \
    } while (0)

int main() {
    const double degs[8] = {0, 8, 8.5, 16, 16.5, 32, 32.5, 1000};
    // word-lanes by window width; wide from 65 words on
    {
        const uint32_t words[10] = {2, 16, 17, 32, 33, 64, 65, 128, 1216, 2048};
        const int lpw[10] = {8, 8, 16, 16, 32, 32, 32, 32, 32, 32};
        const bool wide[10] = {false, false, false, false, false, false, true, true, true, true};
        for (int i = 0; i < 10; i++)
            for (double d : degs) {
                const gossip::PullShape s = gossip::pull_shape(words[i], d);
                CHECK(s.lpw == lpw[i]);
                CHECK(s.wide == wide[i]);
            }
    }
    // edge-lanes by average degree, at one window of each lane count and a wide one
    {
        const uint32_t words[4] = {16, 32, 64, 65};
        const int epn[4][8] = {{1, 1, 2, 2, 4, 4, 8, 8},   // lpw 8
                               {1, 1, 2, 2, 4, 4, 4, 4},   // lpw 16: at most 4
                               {1, 1, 2, 2, 2, 2, 2, 2},   // lpw 32: at most 2
                               {1, 1, 1, 1, 1, 1, 1, 1}};  // wide: one peer walk per node
        for (int i = 0; i < 4; i++)
            for (int k = 0; k < 8; k++) CHECK(gossip::pull_shape(words[i], degs[k]).epn == epn[i][k]);
    }
    // every window a launch can cover
    for (uint32_t w = 1; w <= 2048; w++)
        for (double d : degs) {
            const gossip::PullShape s = gossip::pull_shape(w, d);
            CHECK(s.lpw == 8 || s.lpw == 16 || s.lpw == 32);
            CHECK(s.epn >= 1 && s.lpw * s.epn <= 64);
            CHECK(s.tiles_per_pass() == (uint32_t)s.lpw / 8u);
            CHECK(s.takes_tile_masks() == (s.epn == 1));
            CHECK(s.wide == (w > 64));
            CHECK(!s.wide || (s.lpw == gossip::kWideLanes && s.epn == 1));
        }
    // the per-tick plan: reset clears everything and keeps the vectors' storage
    {
        gossip::TickPlan p;
        p.reset(7, 3);
        p.nb = 5;
        p.snap_idx = 2;
        p.sat_used = true;
        p.new_widx.assign(100, 1);
        p.cb_off.assign(17, 9u);
        p.windows.assign(4, gossip::PullWindow{0u, 16u, gossip::pull_shape(16, 0.0), 1u, 2u, true});
        const uint8_t* w0 = p.new_widx.data();
        const uint32_t* c0 = p.cb_off.data();
        const gossip::PullWindow* pw0 = p.windows.data();
        p.reset(8, 0);
        CHECK(p.t == 8 && p.slot == 0 && p.nb == 0 && p.snap_idx == -1 && !p.sat_used);
        CHECK(p.new_widx.empty() && p.cb_off.empty() && p.windows.empty());
        CHECK(p.new_widx.capacity() >= 100 && p.cb_off.capacity() >= 17 && p.windows.capacity() >= 4);
        p.new_widx.assign(100, 0);
        p.cb_off.assign(17, 0u);
        p.windows.resize(4);
        CHECK(p.new_widx.data() == w0 && p.cb_off.data() == c0 && p.windows.data() == pw0);
    }
    if (fails) {
        std::printf("%d checks FAILED\n", fails);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
