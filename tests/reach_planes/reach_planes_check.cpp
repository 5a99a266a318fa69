// Stand-alone check of the carry-save bit planes of k_reach (csrc/reach_kernel.h: reach_plane_add,
// reach_plane_add4, reach_plane_flush, reach_lane_step), built with -fsanitize=address,undefined by
// tests/test_reach_cpu.py: column counts from the planes against a per-bit loop over the same rows,
// for random, all-ones and all-zero rows, at every row count from 0 to the planes' capacity + 1 and
// at the flush caps the device tests use (1, 3, the capacity).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "reach_kernel.h"

static int fails = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            fails++;                                               \
        }                                                          \
    } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 0x2545f4914f6cdd1dull;
}

enum Kind { RANDOM, SPARSE, ONES, ZEROS, KINDS };

static std::vector<uint64_t> rows_of(Kind k, uint32_t n) {
    std::vector<uint64_t> r(n);
    for (uint32_t i = 0; i < n; i++)
        r[i] = k == RANDOM ? rnd() : k == SPARSE ? (rnd() & rnd() & rnd()) : k == ONES ? ~0ull : 0ull;
    return r;
}

static void per_bit(const std::vector<uint64_t>& rows, uint32_t* want) {
    for (uint32_t b = 0; b < 64; b++) want[b] = 0;
    for (uint64_t x : rows)
        for (uint32_t b = 0; b < 64; b++) want[b] += (uint32_t)((x >> b) & 1ull);
}

static bool same(const uint32_t* a, const uint32_t* b) {
    for (uint32_t k = 0; k < 64; k++)
        if (a[k] != b[k]) return false;
    return true;
}

int main() {
    using namespace gossip;
    CHECK(kReachCap == (1u << kReachPlanes) - 1u);
    // single-row adds, one flush at the end: every count up to the capacity
    for (int kind = 0; kind < KINDS; kind++)
        for (uint32_t n = 0; n <= kReachCap; n++) {
            const std::vector<uint64_t> rows = rows_of((Kind)kind, n);
            uint64_t p[kReachPlanes] = {};
            for (uint64_t x : rows) reach_plane_add(p, x);
            uint32_t got[64] = {}, want[64];
            uint32_t calls = 0;
            for (uint32_t b = 0; b < 64; b++) CHECK(reach_plane_count(p, b) <= n);
            reach_plane_flush(p, [&](uint32_t b, uint32_t c) {
                CHECK(b < 64 && c > 0);
                got[b] += c;
                calls++;
            });
            per_bit(rows, want);
            CHECK(same(got, want));
            if (kind == ZEROS) CHECK(calls == 0);
            if (kind == ONES && n) CHECK(calls == 64 && got[0] == n && got[63] == n);  // the carry chain to plane log2(n)
            for (uint32_t k = 0; k < kReachPlanes; k++) CHECK(p[k] == 0ull);           // flushed planes are empty
        }
    // four-row adds against single-row adds on the same rows (the planes themselves must agree)
    for (int kind = 0; kind < KINDS; kind++)
        for (uint32_t n = 0; n + 4 <= kReachCap; n++) {
            const std::vector<uint64_t> rows = rows_of((Kind)kind, n + 4);
            uint64_t p1[kReachPlanes] = {}, p4[kReachPlanes] = {};
            for (uint32_t i = 0; i < n; i++) {
                reach_plane_add(p1, rows[i]);
                reach_plane_add(p4, rows[i]);
            }
            for (uint32_t i = n; i < n + 4; i++) reach_plane_add(p1, rows[i]);
            reach_plane_add4(p4, rows[n], rows[n + 1], rows[n + 2], rows[n + 3]);
            for (uint32_t k = 0; k < kReachPlanes; k++) CHECK(p1[k] == p4[k]);
        }
    // a lane's loop as k_reach runs it: steps of four rows (missing rows are zeros), flushing at the
    // cap; every row count from 0 to the capacity + 1 at the caps 1, 3 and the capacity, plus a long run
    const uint32_t caps[3] = {1u, 3u, kReachCap};
    for (uint32_t cap : caps)
        for (int kind = 0; kind < KINDS; kind++) {
            std::vector<uint32_t> counts;
            for (uint32_t n = 0; n <= kReachCap + 1; n++) counts.push_back(n);
            counts.push_back(4 * kReachCap + 3);
            for (uint32_t n : counts) {
                const std::vector<uint64_t> rows = rows_of((Kind)kind, n);
                uint64_t p[kReachPlanes] = {};
                uint32_t got[64] = {}, want[64], added = 0, flushes = 0;
                auto add = [&](uint32_t b, uint32_t c) { got[b] += c; };
                auto row = [&](uint32_t i) { return i < n ? rows[i] : 0ull; };
                for (uint32_t i = 0; i < n; i += 4) {
                    const uint32_t before = added;
                    reach_lane_step(p, added, cap, row(i), row(i + 1), row(i + 2), row(i + 3), add);
                    CHECK(added >= 1 && added <= cap);  // never beyond the planes' capacity
                    flushes += added < before + 4 ? 1u : 0u;
                }
                reach_plane_flush(p, add);
                per_bit(rows, want);
                CHECK(same(got, want));
                if (n > cap + 4) CHECK(flushes > 0);  // the run did cross a flush boundary
            }
        }
    if (fails) {
        std::printf("%d checks FAILED\n", fails);
        return 1;
    }
    std::printf("reach planes: all checks passed\n");
    return 0;
}
