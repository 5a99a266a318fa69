// pull_plan.h -- the host's plan of one tick's pull (host only: no HIP, no device code): the launch
// shape of a k_pull launch window, the per-window record and the per-tick plan.  The shape rule
// lives here alone: the tile-list builder, the fold-write decision and the launcher (engine.hip)
// all read the PullShape of a window, none derives it again.
#pragma once

#include <stdint.h>

#include <utility>
#include <vector>

namespace gossip {

// Word-lanes per node of the sparse pull for windows wider than 64 words: 32 (passes of 64 words,
// two nodes per wave step: twice the independent peer chains per wave, and a window never ends in
// a half-idle 128-word pass).  Measured against 64 lanes (profiles/r01/lanes_ab.json: C4 1216
// words 127.7 -> 121.9 ms per launch, the 8-shard 320 words 44.0 -> 36.5 ms, C3 3.35 -> 3.06 ms),
// 16 lanes (C4 128.0 ms) and again in round 4 (64 lanes: C4 phase 69.0 vs 60.4 ms,
// profiles/r04/ab/r4l_*); the option that selected them was removed in round 5.
constexpr int kWideLanes = 32;

// Lane layout of a launch: lpw word-lanes per node (k_pull's LPW: 8, 16 or 32) times epn
// edge-lanes per node (EPN), lpw * epn <= 64.
struct PullShape {
    int lpw;
    int epn;
    bool wide;  // the window holds more than 64 words: several passes, one peer walk per node
    // a pass covers this many 16-word tiles (the tile lists are padded to whole passes)
    uint32_t tiles_per_pass() const { return (uint32_t)lpw / 8u; }
    // tile masks (saturation bits, dense rows, folded rows) run on the gathering kernel only
    bool takes_tile_masks() const { return epn == 1; }
};

// Word-lanes cover the window's words in one pass when possible (at least the 8 word-pairs of one
// tile); spare lanes of the wave split the peer list (edge-lanes) when peers are many.
inline PullShape pull_shape(uint32_t window_words, double avg_deg) {
    int lpw = 8;
    while (lpw < 64 && 2 * lpw < (int)window_words) lpw *= 2;
    if (lpw == 64) return PullShape{kWideLanes, 1, true};
    int epn = 1;
    while (lpw * epn * 2 <= 64 && epn * 8 < avg_deg) epn *= 2;
    return PullShape{lpw, epn, false};
}

// One k_pull launch: kPullLdsWords words of the window (its per-word state lives in LDS).
struct PullWindow {
    uint32_t wb, words;       // the window's words [wb, wb + words)
    PullShape shape;
    uint32_t pt_off, pt_cnt;  // its pass -> tile list in the staging slot's list buffer (use_ptile)
    bool fold;                // some tile of it carries TM_FOLDW / TM_SEENF
};

// What the stages of one tick (engine.hip, tick_step_a) hand to each other.  One per engine, reset
// every tick: the vectors keep their capacity.
struct TickPlan {
    int64_t t = 0;
    int slot = 0;                                         // staging slot
    uint32_t nb = 0, np = 0;                              // staged births / group phases
    uint32_t ny = 0, nwt = 0, ny_read = 0, ny_leave = 0;  // young tiles: all, written, read, leaving
    bool skip_wr = false;           // this tick's slot writers stamp non-empty slots (young_skip)
    std::vector<uint8_t> new_widx;  // per tile: write-sparse index of this tick (0xff: none)
    std::vector<uint32_t> cb_off;   // births of row chunk c: [cb_off[c], cb_off[c + 1])
    int snap_idx = -1;              // the snapshot taken this tick (unbatched runs)
    size_t nsnap = 0;               // hop-batched runs: snapshot masks per word
    bool smask_any = false;         // ... and some mask is set
    bool keep_any = false;    // some word has a keep mask (k_pull stages them in LDS)
    bool group_any = false;   // some word holds an id group (k_dense_fused leaves those ticks to the 3-kernel path)
    bool use_ptile = false;   // k_pull runs over tile lists
    bool sat_used = false;    // ... and keeps saturation bits
    bool dr_used = false;     // ... and reads / writes dense rows
    bool push_on = false;     // push marks ride on the saturation words
    bool pushw_any = false;   // some listed tile is flagged TM_PUSHW
    bool short_any = false;   // some listed tile is flagged TM_SHORT (option pull_batch)
    bool fused_tick = false;  // the tick runs k_dense_fused
    bool nt_rows = false;     // the pull reads and writes rows non-temporally
    int nxt = 0, lv = 0;      // F_next's buffer, the liveness ring entry
    unsigned long long* snap_ptr = nullptr;  // the snapshot's partial count (device)
    std::vector<PullWindow> windows;

    void reset(int64_t tick, int staging_slot) {
        TickPlan fresh;
        fresh.t = tick;
        fresh.slot = staging_slot;
        fresh.new_widx.swap(new_widx);
        fresh.cb_off.swap(cb_off);
        fresh.windows.swap(windows);
        fresh.new_widx.clear();
        fresh.cb_off.clear();
        fresh.windows.clear();
        *this = std::move(fresh);
    }
};

}  // namespace gossip
