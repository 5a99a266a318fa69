// The bit-sliced down-counters of k_rounds (csrc/rounds_kernel.h) as pure host code, checked against per-bit
// integer counters: set / decrement / clear / non-zero for every r in 2..16 over random sequences, and the
// whole word step (rounds_word_step) against a per-column restatement of the rule.  Built with
// -fsanitize=address,undefined by tests/test_rounds_cpu.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "rounds_kernel.h"

using namespace gossip;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// a mask of about 1 / 2^k of the bits
static uint64_t sparse(int k) {
    uint64_t m = ~0ull;
    for (int i = 0; i < k; i++) m &= rnd();
    return m;
}

static long g_checks = 0;
#define CHECK(c)                                                            \
    do {                                                                    \
        g_checks++;                                                         \
        if (!(c)) {                                                         \
            std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)

static void compare(const uint64_t* p, uint32_t np, const uint32_t* ref) {
    uint64_t nzm = 0ull;
    for (uint32_t b = 0; b < 64; b++) {
        CHECK(rounds_plane_count(p, np, b) == ref[b]);
        if (ref[b]) nzm |= 1ull << b;
    }
    CHECK(rounds_plane_nonzero(p, np) == nzm);
    for (uint32_t k = np; k < kRoundsMaxPlanes; k++) CHECK(p[k] == 0ull);  // planes beyond np are never touched
}

int main() {
    CHECK(rounds_planes(1) == 0 && rounds_planes(2) == 1 && rounds_planes(3) == 2 && rounds_planes(4) == 2);
    CHECK(rounds_planes(5) == 3 && rounds_planes(8) == 3 && rounds_planes(9) == 4 && rounds_planes(16) == 4);
    for (uint32_t r = 2; r <= kRoundsMax; r++) {
        const uint32_t np = rounds_planes(r);
        CHECK(np >= 1 && np <= kRoundsMaxPlanes && (1u << np) >= r && (1u << (np - 1)) < r);
        // ---- the three plane functions over random set / decrement / clear sequences ----
        uint64_t p[kRoundsMaxPlanes] = {0, 0, 0, 0};
        uint32_t ref[64] = {0};
        for (int step = 0; step < 4000; step++) {
            const uint64_t op = rnd() % 8;
            if (op < 3) {  // set r - 1 where mask (counters that reached 0 are set again in the same word)
                const uint64_t m = sparse(1 + (int)(rnd() % 4));
                rounds_plane_set(p, np, m, r - 1u);
                for (uint32_t b = 0; b < 64; b++)
                    if ((m >> b) & 1ull) ref[b] = r - 1u;
            } else if (op < 7) {  // decrement where non-zero
                rounds_plane_dec(p, np);
                for (uint32_t b = 0; b < 64; b++)
                    if (ref[b]) ref[b]--;
            } else {  // clear
                const uint64_t m = sparse(2);
                rounds_plane_set(p, np, m, 0u);
                for (uint32_t b = 0; b < 64; b++)
                    if ((m >> b) & 1ull) ref[b] = 0u;
            }
            compare(p, np, ref);
        }
        // every counter runs from r - 1 down to 0 and stays there
        rounds_plane_set(p, np, ~0ull, r - 1u);
        for (uint32_t k = 0; k < r + 2; k++) {
            const uint32_t want = k < r - 1u ? r - 1u - k : 0u;
            for (uint32_t b = 0; b < 64; b += 7) CHECK(rounds_plane_count(p, np, b) == want);
            CHECK(rounds_plane_nonzero(p, np) == (want ? ~0ull : 0ull));
            rounds_plane_dec(p, np);
        }
        // ---- the word step against the rule, column by column ----
        for (uint32_t b = 0; b < 64; b++) ref[b] = 0;
        rounds_plane_set(p, np, ~0ull, 0u);
        uint64_t seen = 0ull;  // a fresh bit is a column the node has not contacted (the pull's rule)
        for (int tick = 0; tick < 3000; tick++) {
            if (rnd() % 64 == 0) {  // the word is retired and re-used: only when nothing is pending
                if (rounds_plane_nonzero(p, np) == 0ull) seen = 0ull;
            }
            const bool down = rnd() % 5 == 0;
            const uint64_t keep = rnd() % 6 == 0 ? rnd() | rnd() : ~0ull;
            const uint64_t fresh = down ? 0ull : sparse(3) & ~seen & keep;  // (a down node has no first contacts)
            seen |= fresh;
            uint64_t old = 0ull;
            const uint64_t S = rounds_word_step(p, np, r, fresh, keep, down, &old);
            uint64_t want_s = 0ull, want_old = 0ull;
            for (uint32_t b = 0; b < 64; b++) {
                const uint64_t bit = 1ull << b;
                const bool alive = (keep & bit) != 0ull;
                const bool resend = ref[b] != 0u && alive && !down;
                if (resend) want_old |= bit;
                if (resend || (fresh & bit)) want_s |= bit;
                if (ref[b]) ref[b]--;               // the round elapses, up or down
                if (fresh & bit) ref[b] = r - 1u;   // r - 1 rounds after this one
                if (!alive) ref[b] = 0u;            // a dead column sends no more
            }
            CHECK(S == want_s && old == want_old && (old & fresh) == 0ull);
            compare(p, np, ref);
        }
    }
    std::printf("rounds planes: %ld checks passed\n", g_checks);
    return 0;
}
