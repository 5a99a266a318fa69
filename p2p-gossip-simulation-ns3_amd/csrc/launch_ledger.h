// launch_ledger.h -- what the engine launched (host only: no HIP, no device code): the key of a
// kernel launch variant, the pure dispatch rule from a k_pull launch's conditions to the
// instantiation that serves it, the list of instantiations that rule can select, and the
// per-engine table of launches by (kernel, variant).  engine.hip's launchers record here from the
// template arguments at their <<<>>> sites, so the table says what was launched, not what a second
// copy of the rule thinks should have been (gossip_engine_get_launches, gossip.h).
#pragma once

#include <stdint.h>

#include <vector>

#include "pull_plan.h"

namespace gossip {

// kernels the ledger records (gossip.h: GOSSIP_K_*)
enum LaunchKernel : uint32_t { LK_PULL = 0, LK_PULL_YOUNG = 1, LK_YOUNG_IDLE = 2, LK_DENSE_BITS = 3, LK_DENSE_DEDUP = 4, LK_REACH = 5, LK_FANOUT = 6, LK_ROUNDS = 7 };
// FROZEN at the ids 0 .. 6 (the kernels up to the thinning path): the fanout ABI tests pin this line, and
// nothing sizes an array by it.  It is not the number of ids -- LK_ROUNDS = 7 follows.
constexpr uint32_t kLaunchKernels = 7;

// k_pull's template flags (gossip.h: GOSSIP_PULL_*)
enum : uint32_t { PK_NT = 1u, PK_SP = 2u, PK_PUSH = 4u, PK_SHORT = 8u, PK_FOLD = 16u };

// A k_pull instantiation <LPW, EPN, NT, SP, PUSH, SHORT, FOLD> as one word: lpw in bits 0-7, epn in
// bits 8-15, the PK_* flags in bits 16-20.  0 is no instantiation (lpw is never 0).
constexpr uint32_t pull_key(int lpw, int epn, bool nt, bool sp, bool push, bool short_batch, bool fold) {
    return (uint32_t)lpw | ((uint32_t)epn << 8) |
           (((nt ? PK_NT : 0u) | (sp ? PK_SP : 0u) | (push ? PK_PUSH : 0u) | (short_batch ? PK_SHORT : 0u) |
             (fold ? PK_FOLD : 0u))
            << 16);
}
constexpr uint32_t pull_key_lpw(uint32_t key) { return key & 0xffu; }
constexpr uint32_t pull_key_epn(uint32_t key) { return (key >> 8) & 0xffu; }
constexpr uint32_t pull_key_flags(uint32_t key) { return (key >> 16) & 0x1fu; }

// The instantiation a k_pull launch runs.  shape: the window's (pull_plan.h); nt: non-temporal
// rows; sp_ok: what the SP instantiations need beside 32 x 1 lanes (tile masks, a pass -> tile list
// of at most kPullMaxPasses passes, saturation words, the seen gate on, no no-skip diagnostic:
// engine.hip pull_sp_ok); push, short_batch, fold: push marks in the launch, a TM_SHORT tile in the
// tick, a folded tile in the window -- read only by the SP instantiations.  0: no instantiation
// serves the shape (lpw not 8, 16 or 32, or lpw x epn above one wave).
constexpr uint32_t pull_dispatch(const PullShape& sh, bool nt, bool sp_ok, bool push, bool short_batch, bool fold) {
    if (sh.lpw != 8 && sh.lpw != 16 && sh.lpw != 32) return 0u;
    if (sh.epn != 1 && sh.epn != 2 && sh.epn != 4 && sh.epn != 8) return 0u;
    if (sh.lpw * sh.epn > 64) return 0u;
    if (sh.lpw == 32 && sh.epn == 1 && sp_ok) return pull_key(32, 1, nt, true, push, short_batch, fold);
    if ((sh.lpw == 32 || sh.lpw == 16) && sh.epn == 1 && nt) return pull_key(sh.lpw, 1, true, false, false, false, false);
    return pull_key(sh.lpw, sh.epn, false, false, false, false, false);
}

// Every instantiation pull_dispatch can select, written out (tests/launch_ledger checks that the
// list and the function agree): the nine lane shapes, the two non-SP non-temporal kernels, and the
// sixteen SP kernels <32, 1, NT?, SP, PUSH?, SHORT?, FOLD?>.
constexpr uint32_t kPullInstantiations = 27;
inline const uint32_t* pull_instantiations() {
    static const uint32_t k[kPullInstantiations] = {
        pull_key(8, 1, 0, 0, 0, 0, 0),  pull_key(8, 2, 0, 0, 0, 0, 0),  pull_key(8, 4, 0, 0, 0, 0, 0),
        pull_key(8, 8, 0, 0, 0, 0, 0),  pull_key(16, 1, 0, 0, 0, 0, 0), pull_key(16, 2, 0, 0, 0, 0, 0),
        pull_key(16, 4, 0, 0, 0, 0, 0), pull_key(32, 1, 0, 0, 0, 0, 0), pull_key(32, 2, 0, 0, 0, 0, 0),
        pull_key(16, 1, 1, 0, 0, 0, 0), pull_key(32, 1, 1, 0, 0, 0, 0),
        pull_key(32, 1, 0, 1, 0, 0, 0), pull_key(32, 1, 0, 1, 0, 0, 1), pull_key(32, 1, 0, 1, 0, 1, 0),
        pull_key(32, 1, 0, 1, 0, 1, 1), pull_key(32, 1, 0, 1, 1, 0, 0), pull_key(32, 1, 0, 1, 1, 0, 1),
        pull_key(32, 1, 0, 1, 1, 1, 0), pull_key(32, 1, 0, 1, 1, 1, 1), pull_key(32, 1, 1, 1, 0, 0, 0),
        pull_key(32, 1, 1, 1, 0, 0, 1), pull_key(32, 1, 1, 1, 0, 1, 0), pull_key(32, 1, 1, 1, 0, 1, 1),
        pull_key(32, 1, 1, 1, 1, 0, 0), pull_key(32, 1, 1, 1, 1, 0, 1), pull_key(32, 1, 1, 1, 1, 1, 0),
        pull_key(32, 1, 1, 1, 1, 1, 1)};
    return k;
}

// "strided" of a launch whose waves loop over work units (64-node chunks for k_pull, k_pull_young and
// k_young_idle, rows for k_dense_dedup): the grid has fewer waves than units, so some wave's loop
// runs more than once.
constexpr bool launch_strides(uint64_t waves, uint64_t units) { return waves < units; }
// "strided" of a k_dense_bits launch: the K split is UNEVEN -- split z takes the stages
// [z * sper, min(nst, (z + 1) * sper)) with sper = ceil(nst / ksplit), so nst % ksplit != 0 gives
// the last non-empty split fewer stages than the others.  That covers the launches with an EMPTY
// split as well: ceil(nst / ksplit) * (ksplit - 1) >= nst is possible only when nst % ksplit != 0.
constexpr bool dense_split_uneven(uint32_t nst, uint32_t ksplit) { return ksplit != 0 && nst % ksplit != 0; }
constexpr bool dense_split_has_empty(uint32_t nst, uint32_t ksplit) {
    return ksplit != 0 && (uint64_t)((nst + ksplit - 1u) / ksplit) * (ksplit - 1u) >= nst;
}

struct LaunchRecord {
    uint32_t kernel;   // LaunchKernel
    uint32_t variant;  // k_pull: pull_key; k_pull_young: its bool template argument; k_dense_bits: ksplit;
                       // k_fanout: 1 / 3 / 5 / 6 the count pass (plain, faults, exact, exact with faults), 2 the compact
                       // pass, 4 the k-th-draw pass; k_rounds: its planes; else 0
    uint64_t launches;
    uint64_t strided;
};

// Launch counts by (kernel, variant), cumulative over an engine's life; a few dozen keys at most,
// kept in first-launch order.
class LaunchLedger {
public:
    void add(LaunchKernel kernel, uint32_t variant, bool strided) {
        for (LaunchRecord& r : recs_)
            if (r.kernel == (uint32_t)kernel && r.variant == variant) {
                r.launches++;
                r.strided += strided ? 1u : 0u;
                return;
            }
        recs_.push_back(LaunchRecord{(uint32_t)kernel, variant, 1u, strided ? 1u : 0u});
    }
    const std::vector<LaunchRecord>& records() const { return recs_; }

private:
    std::vector<LaunchRecord> recs_;
};

}  // namespace gossip
