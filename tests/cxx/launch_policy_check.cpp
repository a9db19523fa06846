// Host check of the chain launch policy (raytracert_amd/csrc/launch_policy.h): the trial tables and their
// schedule, the decision and its margins, the fallback, adoption, the batch order's life launch by launch,
// and the resolved launch shape. No GPU: the header decides, and this program plays rt_capi.cpp's part
// (every event succeeds, every poll finds the last trial ended, as after a synchronising render()).
// Prints "ok <checks>" or the failed checks; run by tests/test_launch_policy.py, also under the host sanitizers.
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

#include "launch_policy.h"

using namespace rt;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        ++g_checks;                                                                   \
        if (!(cond)) { ++g_failed; std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static bool same(const TrialCfg &a, const TrialCfg &b) {
    return a.steal == b.steal && a.dist == b.dist && a.helpers == b.helpers && a.quarter == b.quarter;
}

static void expect_table(int ws, bool auto_dist, int dist, int helpers, int quarter, const std::vector<TrialCfg> &want) {
    TrialCfg t[kMaxTrials];
    const int n = trial_table(ws, auto_dist, dist, helpers, quarter, t);
    CHECK(n == static_cast<int>(want.size()));
    for (int i = 0; i < n && i < static_cast<int>(want.size()); ++i) CHECK(same(t[i], want[i]));
}

// The default knobs (rt_scene's initial values) and their six-candidate table:
// 0 (0,0,1,0)  1 (0,0,1,64)  2 (1,0,1,0)  3 (1,0,1,64)  4 (0,4,1,0)  5 (1,4,1,0)
static ShapeKnobs default_knobs() { return ShapeKnobs{5, 2, 1, -1, 512, 0, 1, 1}; }
// RT_TUNE_SHADOW_HELPERS 2: the nine-candidate table
// 0 (0,0,0,0) 1 (0,0,0,64) 2 (0,0,1,0) 3 (0,0,1,64) 4 (1,0,0,0) 5 (1,0,0,64) 6 (0,4,0,0) 7 (0,4,1,0) 8 (1,4,0,0)
static ShapeKnobs nine_knobs() { ShapeKnobs k = default_knobs(); k.shadow_helpers = 2; return k; }

constexpr uint64_t kSig = 0x1234567;

// Trials with every launch started (`views` frames each), ready to decide.
static TrialState started(const TrialPlan &p, int views = 1) {
    TrialState t;
    t.retarget(kSig, p.key);
    for (int i = 0; i < p.nlaunch; ++i) CHECK(t.begin_trial(views) == i);
    CHECK(t.all_started(p) && !t.decided());
    return t;
}
// Per-launch times from each candidate's two rounds; the warm-up's is `warm`.
static std::vector<float> launch_times(const TrialPlan &p, const std::vector<float> &round1, const std::vector<float> &round2, float warm) {
    std::vector<float> ms(static_cast<size_t>(p.nlaunch), 0.0f);
    ms[0] = warm;
    for (int c = 0; c < p.ncand; ++c) {
        ms[static_cast<size_t>(1 + c)] = round1[static_cast<size_t>(c)];
        ms[static_cast<size_t>(1 + p.ncand + c)] = round2[static_cast<size_t>(c)];
    }
    return ms;
}
static TrialState decide_from(const TrialPlan &p, const std::vector<float> &cand_ms, float warm = 1.0f) {
    TrialState t = started(p);
    const std::vector<float> ms = launch_times(p, cand_ms, cand_ms, warm);
    t.decide(p, ms.data(), p.nlaunch);
    return t;
}

static void check_tables() {
    expect_table(2, true, 0, 1, -1, {{0, 0, 1, 0}, {0, 0, 1, 64}, {1, 0, 1, 0}, {1, 0, 1, 64}, {0, 4, 1, 0}, {1, 4, 1, 0}});
    expect_table(2, true, 0, 2, -1, {{0, 0, 0, 0}, {0, 0, 0, 64}, {0, 0, 1, 0}, {0, 0, 1, 64}, {1, 0, 0, 0}, {1, 0, 0, 64},
                                     {0, 4, 0, 0}, {0, 4, 1, 0}, {1, 4, 0, 0}});
    expect_table(2, true, 0, 2, 0, {{0, 0, 0, 0}, {0, 0, 1, 0}, {1, 0, 0, 0}, {0, 4, 0, 0}, {0, 4, 1, 0}, {1, 4, 0, 0}});
    expect_table(0, false, 0, 1, 0, {{0, 0, 1, 0}});
    expect_table(1, false, 3, 1, 32, {{1, 3, 1, 32}});
    expect_table(0, true, 0, 1, 0, {{0, 0, 1, 0}, {0, 4, 1, 0}});
    expect_table(2, false, 0, 1, 0, {{0, 0, 1, 0}, {1, 0, 1, 0}});
    // trial_plan builds the table the knobs allow: auto only for a fused launch
    CHECK(trial_plan(default_knobs(), true).ncand == 6 && trial_plan(default_knobs(), true).nlaunch == 13);
    CHECK(trial_plan(nine_knobs(), true).ncand == 9 && trial_plan(nine_knobs(), true).nlaunch == 19);
    const TrialPlan unfused = trial_plan(default_knobs(), false);
    CHECK(unfused.ncand == 4 && unfused.cfg[3].dist == 0 && unfused.key != trial_plan(default_knobs(), true).key);

    // trial_key differs whenever any argument of the table differs
    std::set<int> keys;
    int tuples = 0;
    for (int ws = 0; ws <= 2; ++ws)
        for (int a = 0; a <= 1; ++a)
            for (int d = 0; d <= 4; ++d)
                for (int h = 0; h <= 2; ++h)
                    for (int q : {-1, 0, 8, 64, 512}) { keys.insert(trial_key(ws, a != 0, d, h, q)); ++tuples; }
    CHECK(static_cast<int>(keys.size()) == tuples);

    // the launch schedule: a warm-up of candidate 0, then two rounds over the candidates
    CHECK(trial_launches(1) == 0);
    for (int n = 2; n <= kMaxTrials; ++n) {
        CHECK(trial_launches(n) == 1 + 2 * n);
        CHECK(trial_config(0, n) == 0);
        for (int t = 1; t < trial_launches(n); ++t) CHECK(trial_config(t, n) == (t - 1) % n);
    }
    CHECK(trial_launches(kMaxTrials) == kMaxTrialLaunches);
}

static void check_decision() {
    const TrialPlan p = trial_plan(default_knobs(), true);
    {   // the warm-up's time is ignored, whether tiny or huge
        for (float warm : {0.001f, 1000.0f}) {
            const TrialState t = decide_from(p, {1.0f, 1.5f, 0.5f, 1.5f, 1.5f, 1.5f}, warm);
            CHECK(t.choice == 2 && t.ntrial == 6 && same(t.chosen, p.cfg[2]) && t.ms[0] == 1.0f && t.ms[2] == 0.5f);
        }
    }
    {   // the faster of a candidate's two launches counts (in either round)
        TrialState t = started(p);
        std::vector<float> ms = launch_times(p, {1.0f, 1.5f, 1.5f, 2.0f, 1.5f, 0.8f}, {1.0f, 1.5f, 1.5f, 0.5f, 1.5f, 2.0f}, 1.0f);
        t.decide(p, ms.data(), p.nlaunch);
        CHECK(t.choice == 3 && t.ms[3] == 0.5f && t.ms[5] == 0.8f);
    }
    {   // times are divided by the launch's view count
        TrialState t = started(p, 4);
        const std::vector<float> ms = launch_times(p, std::vector<float>(6, 4.0f), std::vector<float>(6, 4.0f), 4.0f);
        t.decide(p, ms.data(), p.nlaunch);
        for (int c = 0; c < 6; ++c) CHECK(t.ms[c] == 1.0f);
        CHECK(t.choice == 0);
        // candidate 2's two launches rendered eight views in the same time: half the time per view
        TrialState u;
        u.retarget(kSig, p.key);
        for (int i = 0; i < p.nlaunch; ++i) u.begin_trial(i > 0 && trial_config(i, p.ncand) == 2 ? 8 : 4);
        u.decide(p, ms.data(), p.nlaunch);
        CHECK(u.choice == 2 && u.ms[2] == 0.5f && u.ms[0] == 1.0f);
    }
    // the 2% rule: a best candidate at 0.985x candidate 0 keeps candidate 0; one at 0.97x is chosen
    CHECK(decide_from(p, {1.0f, 1.5f, 0.985f, 1.5f, 1.5f, 1.5f}).choice == 0);
    CHECK(decide_from(p, {1.0f, 1.5f, 0.97f, 1.5f, 1.5f, 1.5f}).choice == 2);
    {   // plain block dispatch chosen at 1.00; the plain dynamic candidate with the same helpers (4) at 1.02, 1.10, 1.20
        const TrialState a = decide_from(p, {1.0f, 1.5f, 1.5f, 1.5f, 1.02f, 1.5f});
        CHECK(a.choice == 0 && a.inflight_dist == 4 && a.multi_dist == 4);
        const TrialState b = decide_from(p, {1.0f, 1.5f, 1.5f, 1.5f, 1.10f, 1.5f});
        CHECK(b.choice == 0 && b.inflight_dist == 0 && b.multi_dist == 4);
        const TrialState c = decide_from(p, {1.0f, 1.5f, 1.5f, 1.5f, 1.20f, 1.5f});
        CHECK(c.choice == 0 && c.inflight_dist == 0 && c.multi_dist == 0);
        // the quarter-tier block candidate chosen: the same rule (it is the plain kernel too)
        const TrialState d = decide_from(p, {1.0f, 0.5f, 1.5f, 1.5f, 0.55f, 1.5f});
        CHECK(d.choice == 1 && d.inflight_dist == 0 && d.multi_dist == 4);
    }
    {   // a chosen stealing candidate keeps its own distribution for both
        const TrialState a = decide_from(p, {1.0f, 1.5f, 0.5f, 1.5f, 0.505f, 0.51f});
        CHECK(a.choice == 2 && a.chosen.steal == 1 && a.inflight_dist == 0 && a.multi_dist == 0);
        const TrialState b = decide_from(p, {1.0f, 1.5f, 1.5f, 1.5f, 1.5f, 0.5f});
        CHECK(b.choice == 5 && b.chosen.steal == 1 && b.inflight_dist == 4 && b.multi_dist == 4);
        // a chosen dynamic plain candidate: its own, 4
        const TrialState c = decide_from(p, {1.0f, 1.5f, 1.5f, 1.5f, 0.5f, 1.5f});
        CHECK(c.choice == 4 && c.inflight_dist == 4 && c.multi_dist == 4);
    }
    {   // nine candidates: a dynamic candidate with other helpers (6: none) is not counted for a choice with helpers (2)
        const TrialPlan p9 = trial_plan(nine_knobs(), true);
        const TrialState a = decide_from(p9, {1.0f, 1.5f, 0.5f, 1.5f, 1.5f, 1.5f, 0.505f, 0.7f, 1.5f});
        CHECK(a.choice == 2 && a.ntrial == 9 && a.inflight_dist == 0 && a.multi_dist == 0);
        const TrialState b = decide_from(p9, {1.0f, 1.5f, 0.5f, 1.5f, 1.5f, 1.5f, 1.5f, 0.51f, 1.5f});
        CHECK(b.choice == 2 && b.inflight_dist == 4 && b.multi_dist == 4);
    }
    {   // a failed timing (launch 10's could not be read) keeps the first candidate. As in the code this was
        // lifted from, the two distribution rules still run over the times read so far: candidate 4's
        // first-round time is there and within the margins, so both distributions become 4.
        TrialState t = started(p);
        const std::vector<float> ms = launch_times(p, {1.0f, 1.5f, 0.5f, 1.5f, 1.0f, 1.5f}, std::vector<float>(6, 9.0f), 1.0f);
        t.decide(p, ms.data(), 10);
        CHECK(t.choice == 0 && t.ntrial == 6 && same(t.chosen, p.cfg[0]) && t.ms[2] == 0.5f && t.ms[5] == 1.5f && t.ms[3] == 1.5f);
        CHECK(t.inflight_dist == 4 && t.multi_dist == 4);
    }
    {   // the fallback: the first candidate, its distribution for both, the candidate count
        const TrialPlan pf = trial_plan(ShapeKnobs{3, 2, 1, 32, 512, 0, 1, 1}, true);
        CHECK(pf.ncand == 2 && pf.cfg[0].dist == 3);
        TrialState t;
        t.retarget(kSig, pf.key);
        t.begin_trial(1);
        t.settle_first(pf);
        CHECK(t.decided() && t.choice == 0 && t.ntrial == 2 && same(t.chosen, pf.cfg[0]) && t.inflight_dist == 3 && t.multi_dist == 3);
        TrialState u;
        u.retarget(kSig, p.key);
        u.settle_first(p);
        CHECK(u.choice == 0 && u.ntrial == 6 && same(u.chosen, p.cfg[0]) && u.inflight_dist == 0 && u.multi_dist == 0);
    }
    {   // retarget: the same batches and table keep the trials; other batches or another table start them over
        TrialState t = decide_from(p, {1.0f, 1.5f, 0.5f, 1.5f, 1.5f, 1.5f});
        t.retarget(kSig, p.key);
        CHECK(t.choice == 2 && t.n == p.nlaunch);
        t.retarget(kSig + 2, p.key);
        CHECK(t.choice == -1 && t.n == 0 && t.sig == kSig + 2);
        t = decide_from(p, {1.0f, 1.5f, 0.5f, 1.5f, 1.5f, 1.5f});
        t.retarget(kSig, p.key + 1);
        CHECK(t.choice == -1 && t.n == 0);
        t = decide_from(p, {1.0f, 1.5f, 0.5f, 1.5f, 1.5f, 1.5f});
        t.forget();
        CHECK(!t.decided() && t.n == 0 && t.sig == 0 && t.key == -1);
    }
}

static void check_adoption() {
    const TrialPlan p = trial_plan(default_knobs(), true);
    const TrialState a = decide_from(p, {1.0f, 0.5f, 1.5f, 1.5f, 0.55f, 1.5f});
    CHECK(a.choice == 1);
    TrialState b;
    b.retarget(kSig, p.key);
    CHECK(b.adopt(a));
    CHECK(b.choice == a.choice && b.ntrial == a.ntrial && same(b.chosen, a.chosen) && b.inflight_dist == a.inflight_dist &&
          b.multi_dist == a.multi_dist && std::memcmp(b.ms, a.ms, sizeof a.ms) == 0);
    CHECK(b.n == 0);   // (it ran no trial of its own)
    TrialState c;
    c.retarget(kSig + 2, p.key);
    CHECK(!c.adopt(a) && !c.decided());          // other batches
    c.retarget(kSig, p.key + 1);
    CHECK(!c.adopt(a) && !c.decided());          // another table
    c.retarget(kSig, p.key);
    c.begin_trial(1);
    CHECK(!c.adopt(a) && !c.decided());          // it has run a trial
    TrialState undecided = started(p), d;
    d.retarget(kSig, p.key);
    CHECK(!d.adopt(undecided) && !d.decided());  // nothing to adopt
    TrialState e = decide_from(p, {1.0f, 1.5f, 0.5f, 1.5f, 1.5f, 1.5f});
    CHECK(!e.adopt(a) && e.choice == 2);         // it has decided itself
}

// One launch as run_chain and render_tiles book it: (estimated, generation in use, trial index, chain_split,
// re-sort enqueued, deferred sort pending afterwards, decided).
struct Row { int estimated, gen, trial, dist, resort, pending, decided; };
struct View {
    OrderState order;
    TrialState trials;
    ShapeKnobs knobs = default_knobs();
    int order_every = 8;      // RT_TUNE_ORDER_EVERY's default
    bool cold_estimate = true;
    int half = -1;            // the latest launch's half tier

    Row launch(bool moving = false, int views = 1) {
        Row r{};
        if (order.deferred_due()) order.take_deferred();                       // 1. a due deferred order
        bool ordered = order.ordered_for(kSig), estimated = false;
        if (!ordered && cold_estimate) {                                       // 3. a cold order
            order.accept_estimate(kSig);
            ordered = estimated = true;
        }
        const TrialPlan plan = trial_plan(knobs, true);                        // 5. the trials
        int trial = -1;
        bool decided = false;
        if (plan.nlaunch > 0) {
            trials.retarget(kSig, plan.key);
            if (trials.all_started(plan)) {
                const std::vector<float> ms(static_cast<size_t>(plan.nlaunch), 1.0f);
                trials.decide(plan, ms.data(), plan.nlaunch);
            }
            decided = trials.decided();
            if (!decided && trials.wants_trial(plan, ordered && !estimated, order.gen())) trial = trials.begin_trial(views);
        }
        const LaunchShape sh = resolve_shape(knobs, LaunchFacts{ordered, estimated, moving, true, views},   // 4. the shape
                                             decided ? &trials : nullptr, trial >= 0 ? &plan.cfg[trial_config(trial, plan.ncand)] : nullptr);
        half = sh.steal_half;
        r.estimated = estimated;
        r.gen = ordered ? order.gen() : -1;
        r.trial = trial;
        r.dist = sh.chain_split;
        r.resort = order.book_launch(ordered, estimated, moving, order_every);  // 7. booked; render_tiles' sort
        if (r.resort && !order.sort_enqueued(kSig)) order.take_first(kSig);
        r.pending = order.sort_pending;
        r.decided = trials.decided();
        return r;
    }
};

static bool row_is(const Row &r, const Row &w) {
    const bool ok = r.estimated == w.estimated && r.gen == w.gen && r.trial == w.trial && r.dist == w.dist && r.resort == w.resort &&
                    r.pending == w.pending && r.decided == w.decided;
    if (!ok)
        std::printf("  row (%d,%d,%d,%d,%d,%d,%d) expected (%d,%d,%d,%d,%d,%d,%d)\n", r.estimated, r.gen, r.trial, r.dist, r.resort,
                    r.pending, r.decided, w.estimated, w.gen, w.trial, w.dist, w.resort, w.pending, w.decided);
    return ok;
}

static void check_order_life() {
    // A static fused view, the default knobs, after RT_TUNE_FORGET_ORDER. Written down from run_chain and
    // render_tiles: launch 1 runs on the cold estimate and its sort (a re-sort of an order in use, generation
    // 1) is deferred; launch 2 still runs on the estimate (generation 0); launch 3 takes the generation-1
    // order and re-sorts (generation 2); launch 4 waits; launch 5 takes generation 2 and is trial 0. Trials
    // 0..12 are launches 5..17; launch 18 = 6 + 2 x 6 reads them. Once generation 2 is in use a launch with no
    // sort pending counts towards order_every = 8: the eighth such launch (12, then 21) enqueues a deferred
    // re-sort, the next one (13, 22) is not counted, the one after (14, 23) takes it.
    const Row want[] = {
        //est gen trial dist resort pending decided
        {1, 0, -1, 4, 1, 1, 0},   // 1
        {0, 0, -1, 0, 0, 1, 0},   // 2
        {0, 1, -1, 0, 1, 1, 0},   // 3
        {0, 1, -1, 0, 0, 1, 0},   // 4
        {0, 2, 0, 0, 0, 0, 0},    // 5: the warm-up, candidate 0
        {0, 2, 1, 0, 0, 0, 0},    // 6: candidate 0
        {0, 2, 2, 0, 0, 0, 0},    // 7
        {0, 2, 3, 0, 0, 0, 0},    // 8
        {0, 2, 4, 0, 0, 0, 0},    // 9
        {0, 2, 5, 4, 0, 0, 0},    // 10: candidate 4, dynamic
        {0, 2, 6, 4, 0, 0, 0},    // 11
        {0, 2, 7, 0, 1, 1, 0},    // 12: the eighth counted launch re-sorts
        {0, 2, 8, 0, 0, 1, 0},    // 13
        {0, 2, 9, 0, 0, 0, 0},    // 14: takes the re-sorted order
        {0, 2, 10, 0, 0, 0, 0},   // 15
        {0, 2, 11, 4, 0, 0, 0},   // 16
        {0, 2, 12, 4, 0, 0, 0},   // 17: the last trial
        {0, 2, -1, 0, 0, 0, 1},   // 18: decided (all times equal: candidate 0)
        {0, 2, -1, 0, 0, 0, 1},   // 19
        {0, 2, -1, 0, 0, 0, 1},   // 20
        {0, 2, -1, 0, 1, 1, 1},   // 21
        {0, 2, -1, 0, 0, 1, 1},   // 22
        {0, 2, -1, 0, 0, 0, 1},   // 23
    };
    View v;
    for (const Row &w : want) {
        const Row r = v.launch();
        CHECK(row_is(r, w));
        if (!r.estimated) CHECK(v.half == 512);   // (an ordered lone static frame keeps the half tier)
        else CHECK(v.half == 0);
    }
    CHECK(v.trials.choice == 0 && v.trials.inflight_dist == 4 && v.trials.multi_dist == 4);

    // nine candidates: trials at launches 5..23, decided at launch 24 = 6 + 2 x 9
    View n;
    n.knobs = nine_knobs();
    for (int l = 1; l <= 24; ++l) {
        const Row r = n.launch();
        CHECK(r.trial == (l >= 5 && l <= 23 ? l - 5 : -1));
        CHECK(r.decided == (l >= 24));
    }

    // A moving view: every launch that finds no deferred sort waiting re-sorts, so with the deferral every
    // second launch does (from launch 24 on: 23 took the last order), and none keeps the half tier
    const int want_resort[] = {1, 0, 1, 0, 1, 0};
    for (int w : want_resort) {
        const bool waiting = v.order.sort_pending && v.order.pending_age < 1;
        const Row r = v.launch(true);
        CHECK(r.resort == w && r.resort == !waiting && r.gen == 2 && v.half == 0);
    }
    // RT_TUNE_ORDER_EVERY 1 on the static view: the same rhythm
    View e = v;
    e.order_every = 1;
    for (int w : want_resort) {
        (void)w;
        const bool waiting = e.order.sort_pending && e.order.pending_age < 1;
        CHECK(e.launch().resort == !waiting);
    }

    // No cold estimate (RT_TUNE_COLD_ESTIMATE 0): launch 1 has no order and takes dynamic tasks; its sort is
    // the first order, waited for (generation 1, nothing pending); launch 2 runs on it and defers generation
    // 2; launch 4 takes it and is trial 0.
    View c;
    c.cold_estimate = false;
    CHECK(row_is(c.launch(), Row{0, -1, -1, 4, 1, 0, 0}));
    CHECK(c.order.gen() == 1 && c.order.ordered_for(kSig));
    CHECK(row_is(c.launch(), Row{0, 1, -1, 0, 1, 1, 0}));
    CHECK(row_is(c.launch(), Row{0, 1, -1, 0, 0, 1, 0}));
    CHECK(row_is(c.launch(), Row{0, 2, 0, 0, 0, 0, 0}));

    // an adopted order carries its generation: trials at once under generation 2, none under generation 1
    for (int gen : {1, 2}) {
        View a;
        a.order.accept_adopted(kSig, gen);
        const Row r = a.launch();
        CHECK(r.estimated == 0 && r.gen == gen && r.trial == (gen == 2 ? 0 : -1) && r.resort == (gen == 2 ? 0 : 1));
    }

    // forget: the next launch is cold again, on the buffers in use; a new workspace starts from the first ones
    OrderState o = v.order;
    const int cur_order = o.cur_order, cur_cost = o.cur_cost;
    o.since_sort = 5;
    o.forget();
    CHECK(!o.ordered_for(kSig) && o.gen() == 0 && !o.sort_pending && !o.last_ordered && !o.last_measured);
    CHECK(o.cur_order == cur_order && o.cur_cost == cur_cost && o.since_sort == 5);
    o.forget(true);
    CHECK(o.since_sort == 0);
    o = v.order;
    o.rebind();
    CHECK(!o.ordered_for(kSig) && !o.sort_pending && o.cur_order == 0 && o.cur_cost == 0);
}

static bool shape_is(const LaunchShape &s, int split, int steal, int helpers, int quarter, int half, int eighth) {
    const bool ok = s.chain_split == split && s.wave_steal == steal && s.shadow_helpers == helpers && s.steal_quarter == quarter &&
                    s.steal_half == half && s.split_eighth == eighth;
    if (!ok)
        std::printf("  shape (%d,%d,%d,%d,%d,%d) expected (%d,%d,%d,%d,%d,%d)\n", s.chain_split, s.wave_steal, s.shadow_helpers,
                    s.steal_quarter, s.steal_half, s.split_eighth, split, steal, helpers, quarter, half, eighth);
    return ok;
}

static void check_shape() {
    const LaunchFacts measured{true, false, false, true, 1}, cold{false, false, false, true, 1}, estimated{true, true, false, true, 1};
    const LaunchFacts moving{true, false, true, true, 1}, eight{true, false, false, true, 8}, unfused{true, false, false, false, 1};
    // each fixed knob setting passes through (no trials: one candidate)
    for (int split = 0; split <= 4; ++split)
        for (int steal = 0; steal <= 1; ++steal)
            for (int helpers = 0; helpers <= 1; ++helpers)
                for (int quarter : {0, 8}) {
                    const ShapeKnobs k{split, steal, helpers, quarter, 256, 16, 1, 2};
                    CHECK(trial_plan(k, true).nlaunch == 0);
                    for (const LaunchFacts &f : {measured, cold, unfused})
                        CHECK(shape_is(resolve_shape(k, f, nullptr, nullptr), split, steal, helpers, quarter, 256, 16));
                    // a multi-frame, a moving or an estimated launch drops the half and eighth tiers (the fixed quarter tier stays)
                    for (const LaunchFacts &f : {eight, moving, estimated})
                        CHECK(shape_is(resolve_shape(k, f, nullptr, nullptr), split, steal, helpers, quarter, 0, 0));
                }
    // auto, before a decision: a cold or estimated launch takes dynamic tasks (4), an ordered one block dispatch (0);
    // helpers 1 while they are per view; the quarter tier per view is none; wave_steal 2 is the launch-size rule's
    ShapeKnobs k = nine_knobs();
    k.split_eighth = 16;
    TrialState none;
    CHECK(shape_is(resolve_shape(k, cold, nullptr, nullptr), 4, 2, 1, 0, 512, 16));
    CHECK(shape_is(resolve_shape(k, estimated, nullptr, nullptr), 4, 2, 1, 0, 0, 0));
    CHECK(shape_is(resolve_shape(k, measured, nullptr, nullptr), 0, 2, 1, 0, 512, 16));
    CHECK(shape_is(resolve_shape(k, measured, &none, nullptr), 0, 2, 1, 0, 512, 16));   // (undecided trials change nothing)
    CHECK(shape_is(resolve_shape(k, unfused, nullptr, nullptr), 0, 2, 1, 0, 512, 16));  // (auto is a fused launch's)
    CHECK(shape_is(resolve_shape(k, moving, nullptr, nullptr), 0, 2, 1, 0, 0, 0));
    CHECK(shape_is(resolve_shape(k, eight, nullptr, nullptr), 0, 2, 1, 0, 0, 0));
    // during a trial: the candidate's steal, distribution, helpers and quarter tier
    const TrialCfg running{1, 4, 0, 64};
    CHECK(shape_is(resolve_shape(k, measured, nullptr, &running), 4, 1, 0, 64, 512, 16));
    CHECK(shape_is(resolve_shape(k, eight, nullptr, &running), 4, 1, 0, 64, 0, 0));
    // after a decision
    TrialState t;
    t.choice = 1;
    t.chosen = TrialCfg{0, 0, 0, 64};
    t.inflight_dist = 4;
    t.multi_dist = 0;
    CHECK(shape_is(resolve_shape(k, measured, &t, nullptr), 0, 0, 0, 64, 512, 16));           // one frame
    CHECK(shape_is(resolve_shape(k, moving, &t, nullptr), 0, 0, 0, 64, 0, 0));                // (a moving view keeps the quarter tier)
    CHECK(shape_is(resolve_shape(k, estimated, &t, nullptr), 4, 0, 0, 64, 0, 0));             // a new view's cold launch: still dynamic
    CHECK(shape_is(resolve_shape(k, eight, &t, nullptr), 0, 0, 0, 0, 0, 0));                  // eight frames: multi_dist, no split tier
    k.frames_in_flight = 2;
    CHECK(shape_is(resolve_shape(k, measured, &t, nullptr), 4, 0, 0, 64, 512, 16));           // frames in flight: inflight_dist
    CHECK(shape_is(resolve_shape(k, estimated, &t, nullptr), 4, 0, 0, 64, 0, 0));
    t.inflight_dist = 0;
    t.multi_dist = 4;
    CHECK(shape_is(resolve_shape(k, measured, &t, nullptr), 0, 0, 0, 64, 512, 16));
    CHECK(shape_is(resolve_shape(k, eight, &t, nullptr), 4, 0, 0, 0, 0, 0));
    k.inflight_dynamic = 0;                                                                    // RT_TUNE_INFLIGHT_DYNAMIC 0: the choice's own
    t.inflight_dist = 4;
    CHECK(shape_is(resolve_shape(k, measured, &t, nullptr), 0, 0, 0, 64, 512, 16));
    CHECK(shape_is(resolve_shape(k, eight, &t, nullptr), 0, 0, 0, 0, 0, 0));
    // a fixed distribution with trials over stealing alone: the in-flight rule is auto's
    ShapeKnobs f{0, 2, 1, 0, 512, 0, 1, 2};
    t.chosen = TrialCfg{1, 0, 1, 0};
    CHECK(shape_is(resolve_shape(f, measured, &t, nullptr), 0, 1, 1, 0, 512, 0));
    CHECK(shape_is(resolve_shape(f, eight, &t, nullptr), 0, 1, 1, 0, 0, 0));
}

int main() {
    check_tables();
    check_decision();
    check_adoption();
    check_order_life();
    check_shape();
    if (g_failed) {
        std::printf("%d of %d checks failed\n", g_failed, g_checks);
        return 1;
    }
    std::printf("ok %d\n", g_checks);
    return 0;
}
