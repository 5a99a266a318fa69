// Stand-alone check of csrc/launch_ledger.h, built with -fsanitize=address,undefined by
// tests/test_launch_ledger.py: the packing of a k_pull instantiation into a key, the written-out
// list of instantiations against what the dispatch rule can return over all of its inputs, the
// rule itself against a table written out here, the "strided" predicates, and the ledger's counts.
#include <cstdint>
#include <cstdio>
#include <set>

#include "launch_ledger.h"

static int fails = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            fails++;                                               \
        }                                                          \
    } while (0)

using namespace gossip;

int main() {
    // the 27 instantiations, written out once more as (lpw, epn, flags)
    struct Inst { int lpw, epn; uint32_t flags; };
    std::vector<Inst> all;
    const int shapes[9][2] = {{8, 1}, {8, 2}, {8, 4}, {8, 8}, {16, 1}, {16, 2}, {16, 4}, {32, 1}, {32, 2}};
    for (const auto& s : shapes) all.push_back(Inst{s[0], s[1], 0u});
    all.push_back(Inst{32, 1, PK_NT});
    all.push_back(Inst{16, 1, PK_NT});
    for (uint32_t f = 0; f < 16; f++)
        all.push_back(Inst{32, 1, PK_SP | ((f & 1u) ? PK_NT : 0u) | ((f & 2u) ? PK_PUSH : 0u) | ((f & 4u) ? PK_SHORT : 0u) |
                                      ((f & 8u) ? PK_FOLD : 0u)});
    CHECK(all.size() == 27);

    // key packing round-trips; distinct instantiations give distinct non-zero keys
    std::set<uint32_t> want;
    for (const Inst& i : all) {
        const uint32_t k = pull_key(i.lpw, i.epn, i.flags & PK_NT, i.flags & PK_SP, i.flags & PK_PUSH,
                                    i.flags & PK_SHORT, i.flags & PK_FOLD);
        CHECK(k != 0u);
        CHECK(pull_key_lpw(k) == (uint32_t)i.lpw && pull_key_epn(k) == (uint32_t)i.epn && pull_key_flags(k) == i.flags);
        CHECK(want.insert(k).second);
    }
    CHECK(want.size() == 27);

    // the written-out enumeration: 27 distinct keys, the same set
    CHECK(kPullInstantiations == 27);
    std::set<uint32_t> listed(pull_instantiations(), pull_instantiations() + kPullInstantiations);
    CHECK(listed.size() == 27);
    CHECK(listed == want);

    // ... equals the set of keys the dispatch can produce: every lane shape (those the shape rule
    // gives and malformed ones) times every combination of the conditions
    std::set<uint32_t> reached;
    const int lpws[7] = {0, 4, 8, 16, 32, 64, 24}, epns[7] = {0, 1, 2, 3, 4, 8, 16};
    for (int lpw : lpws)
        for (int epn : epns)
            for (uint32_t c = 0; c < 32; c++) {
                const PullShape sh{lpw, epn, false};
                const bool nt = c & 1u, sp_ok = c & 2u, push = c & 4u, sb = c & 8u, fold = c & 16u;
                const uint32_t k = pull_dispatch(sh, nt, sp_ok, push, sb, fold);
                const bool valid = (lpw == 8 || lpw == 16 || lpw == 32) && (epn == 1 || epn == 2 || epn == 4 || epn == 8) &&
                                   lpw * epn <= 64;
                CHECK((k != 0u) == valid);
                if (!k) continue;
                reached.insert(k);
                // the lane shape is never changed; the flags follow the rule, written out
                CHECK(pull_key_lpw(k) == (uint32_t)lpw && pull_key_epn(k) == (uint32_t)epn);
                uint32_t f = 0;
                if (lpw == 32 && epn == 1 && sp_ok)
                    f = PK_SP | (nt ? PK_NT : 0u) | (push ? PK_PUSH : 0u) | (sb ? PK_SHORT : 0u) | (fold ? PK_FOLD : 0u);
                else if ((lpw == 32 || lpw == 16) && epn == 1 && nt)
                    f = PK_NT;
                CHECK(pull_key_flags(k) == f);
            }
    CHECK(reached == listed);
    // every shape the shape rule gives has an instantiation, with and without the conditions
    const double degs[8] = {0, 8, 8.5, 16, 16.5, 32, 32.5, 1000};
    for (uint32_t w = 1; w <= 2048; w++)
        for (double d : degs)
            for (uint32_t c = 0; c < 32; c++) {
                const uint32_t k = pull_dispatch(pull_shape(w, d), c & 1u, c & 2u, c & 4u, c & 8u, c & 16u);
                CHECK(k != 0u && listed.count(k) == 1);
            }
    // a few launches by hand
    CHECK(pull_dispatch(PullShape{32, 1, true}, false, true, true, false, true) == pull_key(32, 1, false, true, true, false, true));
    CHECK(pull_dispatch(PullShape{32, 1, true}, true, false, true, true, true) == pull_key(32, 1, true, false, false, false, false));
    CHECK(pull_dispatch(PullShape{16, 1, false}, true, true, true, true, true) == pull_key(16, 1, true, false, false, false, false));
    CHECK(pull_dispatch(PullShape{8, 1, false}, true, true, false, false, false) == pull_key(8, 1, false, false, false, false, false));
    CHECK(pull_dispatch(PullShape{16, 4, false}, true, true, true, true, true) == pull_key(16, 4, false, false, false, false, false));
    CHECK(pull_dispatch(PullShape{32, 2, false}, true, true, false, false, false) == pull_key(32, 2, false, false, false, false, false));

    // strided: fewer waves than units; the K split: uneven (which includes an empty split)
    CHECK(launch_strides(4, 47) && launch_strides(12, 47) && !launch_strides(48, 47) && !launch_strides(47, 47));
    CHECK(!launch_strides(1, 0) && !launch_strides(4, 1));
    CHECK(dense_split_uneven(9, 4) && dense_split_has_empty(9, 4));    // stages 3 + 3 + 3 + 0
    CHECK(dense_split_uneven(5, 2) && !dense_split_has_empty(5, 2));   // 3 + 2
    CHECK(!dense_split_uneven(8, 4) && !dense_split_has_empty(8, 4));  // 2 + 2 + 2 + 2
    CHECK(!dense_split_uneven(9, 1) && !dense_split_has_empty(9, 1) && !dense_split_uneven(3, 0));
    for (uint32_t nst = 1; nst <= 300; nst++)
        for (uint32_t ks = 1; ks <= 64; ks *= 2) {
            // against the kernel's partition, walked: split z covers [z * sper, min(nst, (z + 1) * sper))
            const uint32_t sper = (nst + ks - 1) / ks;
            uint32_t lo = ~0u, hi = 0, empty = 0, sum = 0;
            for (uint32_t z = 0; z < ks; z++) {
                const uint32_t sb = z * sper, se = sb + sper < nst ? sb + sper : nst;
                const uint32_t len = sb < se ? se - sb : 0;
                sum += len;
                empty += len == 0;
                if (len < lo) lo = len;
                if (len > hi) hi = len;
            }
            CHECK(sum == nst);
            CHECK(dense_split_uneven(nst, ks) == (lo != hi));
            CHECK(dense_split_has_empty(nst, ks) == (empty != 0));
            CHECK(!dense_split_has_empty(nst, ks) || dense_split_uneven(nst, ks));
        }

    // the ledger: counts accumulate per (kernel, variant), records keep first-launch order
    {
        LaunchLedger l;
        CHECK(l.records().empty());
        const uint32_t k0 = pull_key(8, 4, 0, 0, 0, 0, 0), k1 = pull_key(32, 1, 1, 1, 1, 0, 1);
        l.add(LK_PULL, k0, false);
        l.add(LK_PULL, k1, true);
        l.add(LK_PULL, k0, true);
        l.add(LK_PULL_YOUNG, 1u, false);
        l.add(LK_PULL_YOUNG, 0u, true);
        l.add(LK_DENSE_BITS, 4u, true);
        l.add(LK_DENSE_BITS, 1u, false);
        l.add(LK_DENSE_DEDUP, 0u, true);
        l.add(LK_YOUNG_IDLE, 0u, false);
        for (int i = 0; i < 1000; i++) l.add(LK_PULL, k0, i % 2 == 0);
        const std::vector<LaunchRecord>& r = l.records();
        CHECK(r.size() == 8);
        CHECK(r[0].kernel == LK_PULL && r[0].variant == k0 && r[0].launches == 1002 && r[0].strided == 501);
        CHECK(r[1].kernel == LK_PULL && r[1].variant == k1 && r[1].launches == 1 && r[1].strided == 1);
        CHECK(r[2].kernel == LK_PULL_YOUNG && r[2].variant == 1u && r[2].launches == 1 && r[2].strided == 0);
        CHECK(r[3].kernel == LK_PULL_YOUNG && r[3].variant == 0u && r[3].launches == 1 && r[3].strided == 1);
        CHECK(r[4].kernel == LK_DENSE_BITS && r[4].variant == 4u && r[4].strided == 1);
        CHECK(r[5].kernel == LK_DENSE_BITS && r[5].variant == 1u && r[5].strided == 0);
        // (kernel 3, variant 0) and (kernel 4, variant 0) are different keys
        CHECK(r[6].kernel == LK_DENSE_DEDUP && r[6].launches == 1 && r[7].kernel == LK_YOUNG_IDLE && r[7].launches == 1);
        // all 27 instantiations side by side
        LaunchLedger m;
        for (uint32_t rep = 0; rep < 3; rep++)
            for (uint32_t i = 0; i < kPullInstantiations; i++) m.add(LK_PULL, pull_instantiations()[i], rep == 1);
        CHECK(m.records().size() == 27);
        for (const LaunchRecord& x : m.records()) CHECK(x.launches == 3 && x.strided == 1);
    }
    if (fails) {
        std::printf("%d checks FAILED\n", fails);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
