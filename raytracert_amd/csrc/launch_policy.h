// launch_policy.h — where a frame's k_chain launch is placed: which batch order it dispatches by and when
// that order is re-sorted (OrderState), which launch shapes the per-view trials time and which one they
// settle on (TrialState), and the shape one launch takes (resolve_shape). Placement only: no rule here
// changes a pixel. Nothing in this header touches HIP: it decides, rt_capi.cpp enqueues (the order and
// duration buffers, the streams and the events stay in its Pipe), so tests/cxx/launch_policy_check.cpp
// drives every rule on the host.
#pragma once

#include <algorithm>
#include <cstdint>

#include "raytracert_tune.h"   // RT_MAX_TRIALS

namespace rt {

// The per-view launch trials (RT_TUNE_WAVE_STEAL 2, RT_TUNE_CHAIN_SPLIT 5, RT_TUNE_SHADOW_HELPERS 2):
// trial t of a batch geometry runs configuration t of this table, in this order.
// Trial launches: a warm-up launch of candidate 0 (the first launch after a new batch order measured
// slow in every workload), then two rounds over the candidates; each candidate's time is the faster
// of its two launches. The choice is the fastest candidate, unless within 2% of candidate 0 (plain
// kernel, first distribution, no helpers): single launches carry a few % of noise, so a near tie
// keeps the simplest shape.
constexpr int kMaxTrials = RT_MAX_TRIALS;          // candidates
constexpr int kMaxTrialLaunches = 1 + 2 * kMaxTrials;
constexpr float kTrialMargin = 0.98f;
constexpr int kQuarterTrial = 64;   // RT_TUNE_STEAL_QUARTER -1 (per view): the quarter tier the trials time against none
struct TrialCfg { int steal, dist, helpers, quarter; };
// The candidate table: per distribution (block dispatch 0, then dynamic 4 when auto), the plain kernel
// (without, then with shadow helpers when they are per view) and the stealing kernel; with the quarter
// tier per view (steal_quarter -1) the block-dispatch candidates also run with the longest 64 batches
// as quarter waves (r03: ref_default 0.562 -> 0.509 ms, C3 0.215 -> 0.198, C2 0.158 -> 0.166, C4 equal).
inline int trial_table(int wave_steal, bool auto_dist, int dist, int shadow_helpers, int steal_quarter, TrialCfg (&t)[kMaxTrials]) {
    int n = 0;
    for (int d = 0; d < (auto_dist ? 2 : 1); ++d) {
        const int dd = auto_dist ? (d ? 4 : 0) : dist;
        for (int st = 0; st < (wave_steal == 2 ? 2 : 1); ++st) {
            const int steal = wave_steal == 2 ? st : wave_steal;
            for (int h = 0; h < (shadow_helpers == 2 && steal != 1 ? 2 : 1); ++h) {
                const int helpers = shadow_helpers == 2 ? (steal == 1 ? 0 : h) : shadow_helpers;
                const int nq = (steal_quarter < 0 && dd == 0) ? 2 : 1;
                for (int q = 0; q < nq && n < kMaxTrials; ++q)
                    t[n++] = TrialCfg{steal, dd, helpers, steal_quarter < 0 ? (q ? kQuarterTrial : 0) : steal_quarter};
            }
        }
    }
    return n;
}
// The knobs a trial table is built from, as one key: a decision stands only for the table it was made on.
inline int trial_key(int wave_steal, bool auto_dist, int dist, int shadow_helpers, int steal_quarter) {
    return wave_steal | (auto_dist ? 4 : 0) | (dist << 3) | (shadow_helpers << 6) | ((steal_quarter < 0 ? 1 : 0) << 8) |
           ((steal_quarter < 0 ? 0 : steal_quarter) << 9);
}
inline int trial_launches(int candidates) { return candidates > 1 ? 1 + 2 * candidates : 0; }
inline int trial_config(int launch, int candidates) { return launch == 0 ? 0 : (launch - 1) % candidates; }

// With frames in flight, dynamic wave tasks on a resident grid let the next frame's
// blocks take the slots the previous frame's tail frees (block dispatch runs two
// frames side by side from their first blocks, profiles/r04_ab_inflight.txt): taken
// for the plain kernel when its distribution-4 candidate timed within 3% of the choice
// alone (C4: 0.387 -> 0.377 ms per frame two in flight). C3, whose distribution-4
// candidate is ~20% slower alone, and the stealing kernel (ref_default: 0.26 -> 0.30 ms
// in flight with distribution 4 even where the trials timed both alike) keep theirs.
constexpr float kInflightDynamicMargin = 1.03f;
// A multi-frame launch takes dynamic wave tasks unless they timed far slower alone:
// the 3% rule decides by a single launch's noise, and a block-dispatch launch of
// eight C4 camera-path views measured 4% slower (0.324-0.330 ms per frame against
// 0.310-0.317; its dynamic candidate timed 1.01-1.07x the choice alone); C3's
// dynamic candidate times 1.3x alone and its multi-frame launch 1.22x
// (profiles/r06u_ab_multiframe_knobs.txt, r06w_ab_multi_dynamic.txt, r06x_ab_workloads.txt)
constexpr float kMultiDynamicMargin = 1.15f;

// The scene's knobs that shape a chain launch, as rt_scene_tune stores them (chain_split 5: auto;
// wave_steal 2 and shadow_helpers 2: per view; steal_quarter -1: per view).
struct ShapeKnobs {
    int chain_split, wave_steal, shadow_helpers, steal_quarter, steal_half, split_eighth;
    int inflight_dynamic, frames_in_flight;
};

// The trial table of one launch: the candidates the knobs allow, its key and its launch count
// (0: one candidate, nothing to time). fused: the launch writes the pixels (one fused frame batch).
struct TrialPlan {
    TrialCfg cfg[kMaxTrials];
    int ncand = 0, key = 0, nlaunch = 0;
};
inline TrialPlan trial_plan(const ShapeKnobs &k, bool fused) {
    TrialPlan p;
    const bool auto_dist = k.chain_split == 5 && fused;
    const int dist = k.chain_split == 5 ? 0 : k.chain_split;
    p.ncand = trial_table(k.wave_steal, auto_dist, dist, k.shadow_helpers, k.steal_quarter, p.cfg);
    p.key = trial_key(k.wave_steal, auto_dist, dist, k.shadow_helpers, k.steal_quarter);
    p.nlaunch = trial_launches(p.ncand);
    return p;
}

// One pipeline's launch trials.
// RT_TUNE_WAVE_STEAL 2 (auto): the first chain launches over a batch geometry that dispatch
// by a MEASURED batch order run without and with in-wave stealing between event pairs (the same
// order quality for both: an estimated order would favour whichever trial ran second); once
// all have completed (polled, never waited for), later launches over that geometry use the
// faster. Before that, the launch-size rule. Placement only.
// With RT_TUNE_CHAIN_SPLIT 5 (auto) the trials also cover the distribution (0: hardware block
// dispatch, 4: dynamic wave tasks): up to four trials (steal x distribution), the fastest kept.
// RT_TUNE_SHADOW_HELPERS 2 (auto) adds the shadow-helper choice to the non-stealing trials (up
// to six candidates: per distribution, plain without and with helpers, stealing; trial_table),
// timed twice each after a warm-up launch (trial_launches).
struct TrialState {
    uint64_t sig = 0;                     // the batch geometry the trials run (or ran) on
    int key = -1;                         // trial_key of the table the trials ran (or run) on
    int n = 0;                            // trial launches started
    int choice = -1;                      // the decided candidate's index (-1: none yet)
    int ntrial = 0;                       // candidates of the table it was decided on
    TrialCfg chosen{};                    // the decided candidate (valid when choice >= 0)
    int inflight_dist = 0;                // its distribution with frames in flight (RT_TUNE_INFLIGHT_DYNAMIC)
    int multi_dist = 0;                   // ... and in a multi-frame launch
    float ms[kMaxTrials] = {};            // each candidate's chain-launch time (rt_scene_trials)
    int frames[kMaxTrialLaunches] = {};   // views in each trial launch (multi-frame: time per view)

    bool decided() const { return choice >= 0; }

    // new batches, or knobs changed since: the trials start over
    void retarget(uint64_t new_sig, int new_key) {
        if (sig == new_sig && key == new_key) return;
        sig = new_sig; key = new_key; n = 0; choice = -1;
    }
    // Every trial dropped (forget_orders): the next fused launch retargets.
    void forget() { sig = 0; key = -1; n = 0; choice = -1; }

    // another pipeline decided for these batches: adopt it (its trials ran without a frame in flight
    // beside them). Only before this pipeline has run a trial of its own. Returns whether it adopted.
    bool adopt(const TrialState &o) {
        if (choice >= 0 || n != 0 || o.sig != sig || o.key != key || o.choice < 0) return false;
        choice = o.choice;
        ntrial = o.ntrial;
        chosen = o.chosen;
        inflight_dist = o.inflight_dist;
        multi_dist = o.multi_dist;
        for (int c = 0; c < kMaxTrials; ++c) ms[c] = o.ms[c];
        return true;
    }

    // Settle on the first candidate without (or despite) the timings: a trial that could not be started
    // or closed. The candidates' times are left as they are.
    void settle_first(const TrialPlan &p) {
        choice = 0;
        ntrial = p.ncand;
        chosen = p.cfg[0];
        inflight_dist = multi_dist = p.cfg[0].dist;
    }

    // This launch runs a trial: not decided, launches left, and the launch dispatches by an order measured
    // under a measured order (generation 2: orders converge over the first re-sorts).
    bool wants_trial(const TrialPlan &p, bool measured_order, int order_gen) const {
        return choice < 0 && n < p.nlaunch && measured_order && order_gen >= 2;
    }
    // The trial this launch runs (its start event is recorded): its index; `views` frames in the launch.
    int begin_trial(int views) {
        frames[n] = std::max(1, views);
        return n++;
    }
    // Every trial launch has been started (the caller then polls the last one's end event).
    bool all_started(const TrialPlan &p) const { return choice < 0 && n >= p.nlaunch; }

    // Decide from the trial launches' times: launch_ms[t] is launch t's, for 1 <= t < timed (launch 0, the
    // warm-up, is not read). timed == p.nlaunch: all were read; fewer: reading launch `timed` failed, and
    // the first candidate is kept (a failed timing). Times are per view; a candidate's is the faster of its
    // two launches; the fastest wins unless within kTrialMargin of candidate 0.
    // (As in the code this was lifted from, the two distribution rules below also run after a failed
    // timing, over the times read so far.)
    void decide(const TrialPlan &p, const float *launch_ms, int timed) {
        choice = 0;   // (a failed timing: keep the first candidate)
        ntrial = p.ncand;
        for (int c = 0; c < p.ncand; ++c) ms[c] = 0;
        for (int t = 1; t < std::min(timed, p.nlaunch); ++t) {
            const float v = launch_ms[t] / static_cast<float>(std::max(1, frames[t]));
            float &m = ms[trial_config(t, p.ncand)];
            m = m == 0 ? v : std::min(m, v);
        }
        if (timed >= p.nlaunch) {
            int best = 0;
            for (int c = 1; c < p.ncand; ++c)
                if (ms[c] < ms[best]) best = c;
            choice = (best != 0 && ms[best] > kTrialMargin * ms[0]) ? 0 : best;
        }
        chosen = p.cfg[choice];
        inflight_dist = multi_dist = chosen.dist;
        for (int c = 0; c < p.ncand; ++c)
            if (p.cfg[c].dist == 4 && chosen.steal == 0 && p.cfg[c].steal == 0 && p.cfg[c].helpers == chosen.helpers && ms[c] > 0) {
                if (ms[c] <= kInflightDynamicMargin * ms[choice]) inflight_dist = 4;
                if (ms[c] <= kMultiDynamicMargin * ms[choice]) multi_dist = 4;
            }
    }
};

// One pipeline's batch-order bookkeeping. The buffers themselves (Pipe::order_buf, Pipe::cost_buf) are
// double-buffered: a launch's measured durations (cost buffer cur_cost) are sorted on
// the side stream into order buffer cur_order ^ 1 while the next launch still dispatches by
// order buffer cur_order and writes its durations into the other cost buffer; the launch after
// that waits for the sort (long done by then) and switches to the new order. No launch ever
// reads an order buffer a sort is writing, nor writes a cost buffer a sort is reading.
// The first sort for a batch geometry (no order for it yet) is waited for at once.
struct OrderState {
    uint64_t buf_sig[2] = {0, 0};   // batch geometry whose order each buffer holds (0: none)
    // where each buffer's order came from: 0 the cold estimate, 1 durations measured by a launch
    // without a measured order (a cold launch), 2 durations of a launch dispatched by a measured
    // order (what the launch trials wait for: orders converge over the first re-sorts)
    int buf_gen[2] = {0, 0};
    int cur_cost = 0, cur_order = 0;
    bool sort_pending = false;      // a deferred sort into order buffer cur_order ^ 1
    int pending_age = 0;            // launches since it was enqueued
    uint64_t pending_sig = 0;
    int pending_gen = 0;            // the generation of the deferred sort's order
    int since_sort = 0;             // launches over these batches since their order was last sorted
    bool last_ordered = false;      // the latest booked launch dispatched by an order for its batches, estimated or measured:
                                    // its sort is a re-sort (deferred), not a first order (waited for)
    bool last_measured = false;     // ... and that order was not this launch's own cold estimate: its sort's order is generation 2

    bool ordered_for(uint64_t sig) const { return buf_sig[cur_order] == sig; }
    int gen() const { return buf_gen[cur_order]; }

    // a deferred re-sort: the launch after the one that enqueued it switches to it. Counts this launch.
    bool deferred_due() { return sort_pending && pending_age++ >= 1; }
    void take_deferred() {
        cur_order ^= 1;
        buf_sig[cur_order] = pending_sig;
        buf_gen[cur_order] = pending_gen;
        sort_pending = false;
    }
    // The current buffer now holds another pipeline's order for `sig` (copied), of generation `gen`, so the
    // trials and the re-sort schedule continue where that pipeline is.
    void accept_adopted(uint64_t sig, int gen) { buf_sig[cur_order] = sig; buf_gen[cur_order] = gen; }
    // ... or the cold estimate for `sig`.
    void accept_estimate(uint64_t sig) { buf_sig[cur_order] = sig; buf_gen[cur_order] = 0; }

    // A launch over orderable batches was enqueued: does it re-sort? While a deferred sort waits, nothing
    // is booked. Otherwise re-sorted every order_every launches (durations change slowly);
    // measured beats estimated; until an order measured under a measured order is in use,
    // every launch re-sorts; so does a moving view's.
    bool book_launch(bool ordered, bool estimated, bool moving, int order_every) {
        if (sort_pending) return false;
        bool resort = false;
        if (!ordered || estimated || gen() < 2 || ++since_sort >= order_every || moving) {
            resort = true;
            since_sort = 0;
        }
        last_ordered = ordered;
        last_measured = ordered && !estimated;
        return resort;
    }
    // The booked launch's sort was enqueued (from cost buffer cur_cost into order buffer cur_order ^ 1):
    // later launches write their durations into the other buffer. A re-sort is deferred: the launch
    // after next switches to it (no stall); returns whether it was. Else the caller waits for the sort
    // and calls take_first.
    bool sort_enqueued(uint64_t sig) {
        cur_cost ^= 1;
        if (last_ordered) {
            sort_pending = true;
            pending_age = 0;
            pending_sig = sig;
            pending_gen = last_measured ? 2 : 1;
        }
        return sort_pending;
    }
    // the first order for these batches: waited for now
    void take_first(uint64_t sig) {
        cur_order ^= 1;
        buf_sig[cur_order] = sig;
        buf_gen[cur_order] = 1;
    }

    // Every order dropped (RT_TUNE_FORGET_ORDER): the next launch over any batches is cold. The buffers in
    // use stay the ones they are. new_geometry (rt_scene_set_mesh): the re-sort count starts over too.
    void forget(bool new_geometry = false) {
        buf_sig[0] = buf_sig[1] = 0;
        buf_gen[0] = buf_gen[1] = 0;
        sort_pending = false;
        last_ordered = last_measured = false;
        if (new_geometry) since_sort = 0;
    }
    // A new workspace: its buffers hold nothing, and the first of each is in use.
    void rebind() {
        forget();
        cur_cost = cur_order = 0;
    }
};

// What one launch is: dispatched by an order for its batches (ordered), that order being its own cold
// estimate (estimated), a moving view's, a fused frame's, and how many views it renders.
struct LaunchFacts {
    bool ordered, estimated, moving, fused;
    int frames;
};
// What launch_chain is told (DevScene's fields of these names).
struct LaunchShape { int chain_split, wave_steal, shadow_helpers, steal_quarter, steal_half, split_eighth; };

// The shape of one launch. trials: the pipeline's trials when this launch is under them (a fused frame of
// a pipeline, a table of more than one candidate), else null; running: the candidate this launch times,
// else null.
inline LaunchShape resolve_shape(const ShapeKnobs &k, const LaunchFacts &f, const TrialState *trials, const TrialCfg *running) {
    // (5, auto: 0 or 4 per launch; -1, per view: the trials' choice)
    LaunchShape sh{k.chain_split == 5 ? 0 : k.chain_split, k.wave_steal, k.shadow_helpers, std::max(0, k.steal_quarter),
                   k.steal_half, k.split_eighth};
    const bool measured = f.ordered && !f.estimated, multi_frames = f.frames > 1;
    // RT_TUNE_CHAIN_SPLIT 5 (auto): a cold launch (no measured order) takes its wave batches
    // dynamically (4: no wave slot waits for its block to retire while the long batches of an
    // unordered launch trail); ordered launches take the trials' choice, else block dispatch
    const bool auto_dist = k.chain_split == 5 && f.fused;
    if (auto_dist) sh.chain_split = measured ? 0 : 4;
    // The split tiers (half waves for the longest batches, which shorten a lone frame's critical path)
    // only for one frame under an order measured on this very view: a cold launch's centre-out estimate
    // and a moving view's dilated order do not know which batches are the longest, and a multi-frame
    // launch's longest batches overlap the other frames' work anyway, so there the splits only cost wave
    // slots (r06, C4: eight camera-path views per call 0.321-0.323 -> 0.310-0.316 ms per frame, eight
    // copies of the static view 0.3187-0.3228 -> 0.3091-0.3093, orbit one at a time 0.430 -> 0.426,
    // cold frame 0.529-0.552 -> 0.503-0.531; one static frame at a time keeps them: 0.36 against 0.41
    // without; profiles/r06q_ab_split_half.txt, r06r_ab_split_settled.txt, r06s_ab_split_multi.txt)
    // (the eighth tier, off by default, follows the same rule: set for every launch it cost the eight-view
    // line 3-12%, profiles/r06al_ab_split_tiers_lone.txt)
    if (f.estimated || f.moving || multi_frames) sh.steal_half = sh.split_eighth = 0;
    if (k.shadow_helpers == 2) sh.shadow_helpers = 1;   // (until the trials decide)
    if (trials && trials->decided()) {
        const TrialCfg &c = trials->chosen;
        sh.wave_steal = c.steal;
        sh.shadow_helpers = c.helpers;
        // The quarter tier is a split tier: a lone frame's, like the half tier above (multi-frame
        // launches without it: C3 0.131-0.133 -> 0.128 ms per frame, ref_default 0.145-0.149 ->
        // 0.134-0.144, C2 0.032 -> 0.030, C4 equal; profiles/r06y_ab_quarter_multi.txt)
        sh.steal_quarter = multi_frames ? 0 : c.quarter;
        if (measured) sh.chain_split = c.dist;
        // frames in flight: dynamic wave tasks on a resident grid (4) whatever the one-in-flight
        // trials chose. Two block-dispatch launches on two queues share the CUs from their
        // first blocks on and end together (both frames' longest batches stretched side by
        // side); a resident grid's blocks hold their slots until the tasks run out, so the
        // next frame's blocks take the slots the previous frame's tail frees. C4 two in flight
        // 0.39-0.42 -> 0.362-0.365 ms per frame (profiles/r04_ab_inflight.txt)
        if (measured && auto_dist && k.inflight_dynamic && (k.frames_in_flight > 1 || multi_frames))
            sh.chain_split = multi_frames ? trials->multi_dist : trials->inflight_dist;
    } else if (running) {   // trial t runs configuration t of trial_table
        sh.wave_steal = running->steal;
        sh.chain_split = running->dist;
        sh.shadow_helpers = running->helpers;
        sh.steal_quarter = running->quarter;
    }
    return sh;
}

}  // namespace rt
