// fanout_rule_check.cpp -- the fanout selection rule of csrc/fanout_kernel.h as pure host code: reads
// "seed sender receiver copy tick thr expected" lines (decimal) from the file named on the command
// line, checks gossip::fanout_selected on each, then the threshold formula on a few fixed points.
// Built with -fsanitize=address,undefined by tests/test_fanout_cpu.py.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "fanout_kernel.h"

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: fanout_rule_check VECTORS\n");
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    uint64_t seed, tick;
    uint32_t u, v, c, thr;
    int want;
    size_t n = 0, bad = 0;
    std::vector<uint64_t> first_bad;
    while (std::fscanf(f, "%" SCNu64 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu64 " %" SCNu32 " %d", &seed, &u, &v, &c, &tick,
                       &thr, &want) == 7) {
        const int got = gossip::fanout_selected(seed, u, v, c, (uint32_t)tick, thr) ? 1 : 0;
        if (got != want && bad++ == 0) first_bad = {seed, u, v, c, tick, thr};
        n++;
    }
    std::fclose(f);
    if (bad) {
        std::printf("%zu of %zu vectors differ, first: seed %" PRIu64 " %" PRIu64 " -> %" PRIu64 " copy %" PRIu64 " tick %" PRIu64
                    " thr %" PRIu64 "\n",
                    bad, n, first_bad[0], first_bad[1], first_bad[2], first_bad[3], first_bad[4], first_bad[5]);
        return 1;
    }
    // thresholds: always at or below k, floor(k * 2^32 / deg) above
    size_t tbad = 0;
    tbad += gossip::fanout_threshold(3, 0) != 0xffffffffu;
    tbad += gossip::fanout_threshold(3, 3) != 0xffffffffu;
    tbad += gossip::fanout_threshold(3, 4) != 0xC0000000u;
    tbad += gossip::fanout_threshold(1, 2) != 0x80000000u;
    tbad += gossip::fanout_threshold(1, 3) != 0x55555555u;
    tbad += gossip::fanout_threshold(0xfffffffeu, 0xffffffffu) != 0xfffffffeu;
    // "k deg expected" lines of the second file, if given
    size_t nt = 6;
    if (argc > 2) {
        std::FILE* g = std::fopen(argv[2], "r");
        if (!g) {
            std::perror(argv[2]);
            return 2;
        }
        uint32_t k, deg, want_thr;
        while (std::fscanf(g, "%" SCNu32 " %" SCNu32 " %" SCNu32, &k, &deg, &want_thr) == 3) {
            tbad += gossip::fanout_threshold(k, deg) != want_thr;
            nt++;
        }
        std::fclose(g);
    }
    if (tbad) {
        std::printf("%zu threshold points differ\n", tbad);
        return 1;
    }
    std::printf("%zu vectors, %zu thresholds: checks passed\n", n, nt);
    return n ? 0 : 1;
}
