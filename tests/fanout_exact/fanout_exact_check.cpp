// fanout_exact_check.cpp -- the exact-k selection rule of csrc/fanout_kernel.h as pure host code.
//   argv[1]  rows from the model: "seed sender k tick D" and then D times "receiver copy draw selected" (decimal);
//            gossip::fanout_exact_row must give the same draws and the same selection, and report the number
//            selected.
//   argv[2]  hand-made draws for gossip::fanout_exact_bound: "k D" then D draws, then "bound count"; the bound
//            and the count must match, and for k > 0 exactly `count` draws must pass gossip::fanout_exact_pass.
// Built with -fsanitize=address,undefined by tests/test_fanout_exact_cpu.py.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "fanout_kernel.h"

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: fanout_exact_check ROWS BOUNDS\n");
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    uint64_t seed, tick;
    uint32_t sender, k, D;
    size_t rows = 0, copies = 0, bad = 0;
    while (std::fscanf(f, "%" SCNu64 " %" SCNu32 " %" SCNu32 " %" SCNu64 " %" SCNu32, &seed, &sender, &k, &tick, &D) == 5) {
        std::vector<uint32_t> recv(D), copy(D);
        std::vector<uint64_t> want_w(D), got_w(D), work((size_t)D + (k < D ? k : D));
        std::vector<uint8_t> want_s(D), got_s(D);
        uint32_t want_n = 0;
        for (uint32_t i = 0; i < D; i++) {
            unsigned s = 0;
            if (std::fscanf(f, "%" SCNu32 " %" SCNu32 " %" SCNu64 " %u", &recv[i], &copy[i], &want_w[i], &s) != 4) {
                std::fprintf(stderr, "row %zu: short\n", rows);
                return 2;
            }
            want_s[i] = (uint8_t)s;
            want_n += s;
        }
        const uint32_t n = gossip::fanout_exact_row(seed, sender, D, recv.data(), copy.data(), k, (uint32_t)tick, got_s.data(),
                                                    got_w.data(), work.data());
        bool ok = n == want_n;
        for (uint32_t i = 0; i < D; i++) ok = ok && got_w[i] == want_w[i] && got_s[i] == want_s[i];
        if (!ok && bad++ == 0)
            std::printf("first differing row: %zu (seed %" PRIu64 " sender %" PRIu32 " k %" PRIu32 " tick %" PRIu64 " D %" PRIu32
                        "): %" PRIu32 " selected, model %" PRIu32 "\n", rows, seed, sender, k, tick, D, n, want_n);
        rows++;
        copies += D;
    }
    std::fclose(f);
    if (bad) {
        std::printf("%zu of %zu rows differ\n", bad, rows);
        return 1;
    }
    std::FILE* g = std::fopen(argv[2], "r");
    if (!g) {
        std::perror(argv[2]);
        return 2;
    }
    size_t bounds = 0, bbad = 0;
    while (std::fscanf(g, "%" SCNu32 " %" SCNu32, &k, &D) == 2) {
        std::vector<uint64_t> w(D), keep(k < D ? k : D);
        for (uint32_t i = 0; i < D; i++)
            if (std::fscanf(g, "%" SCNu64, &w[i]) != 1) return 2;
        uint64_t want_b;
        uint32_t want_c, count = 0xdeadu;
        if (std::fscanf(g, "%" SCNu64 " %" SCNu32, &want_b, &want_c) != 2) return 2;
        const uint64_t b = gossip::fanout_exact_bound(w.data(), D, k, keep.data(), &count);
        uint32_t pass = 0;
        for (uint32_t i = 0; i < D; i++) pass += gossip::fanout_exact_pass(w[i], b) ? 1u : 0u;
        const bool ok = b == want_b && count == want_c && (k == 0 || pass == count);
        if (!ok) {
            std::printf("bound case %zu (k %" PRIu32 ", D %" PRIu32 "): bound %" PRIu64 " count %" PRIu32 " passing %" PRIu32
                        ", expected %" PRIu64 " %" PRIu32 "\n", bounds, k, D, b, count, pass, want_b, want_c);
            bbad++;
        }
        bounds++;
    }
    std::fclose(g);
    // the compare at its ends
    size_t cbad = 0;
    cbad += !gossip::fanout_exact_pass(0ull, 0ull);
    cbad += gossip::fanout_exact_pass(1ull, 0ull);
    cbad += !gossip::fanout_exact_pass(0ull, gossip::kFanoutExactAll);
    cbad += !gossip::fanout_exact_pass(~0ull, gossip::kFanoutExactAll);
    cbad += gossip::fanout_exact_pass(~0ull, ~0ull - 1ull);
    cbad += !gossip::fanout_exact_pass(~0ull - 1ull, ~0ull - 1ull);
    if (bbad || cbad) {
        std::printf("%zu bound cases, %zu compare points differ\n", bbad, cbad);
        return 1;
    }
    std::printf("%zu rows, %zu copies, %zu bounds: checks passed\n", rows, copies, bounds);
    return rows && bounds ? 0 : 1;
}
