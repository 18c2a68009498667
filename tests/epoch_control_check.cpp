// The engine-side control of the resident search (dbgsom_amd/csrc/epoch_control.h) on the CPU, held against the text
// it replaced: the inline logic of engine.hip at commit 2d7f700, transcribed below as plain functions over a plain
// struct of the fields dbgsom_ctx had then (Legacy, legacy_*).  The transcription is the oracle.
//   epoch_control_check enumerate   every input of the two decisions, both sides, field by field; prints the counts
//   epoch_control_check sequences   both sides in lockstep over event sequences, compared after every step
//   epoch_control_check scenario    commands on stdin, one line of output each (tests/test_epoch_control_cpu.py):
//       epoch M LISTS GROUPS HANDED   one epoch of the pruning arm on the cheap seeds; LISTS: the mean list, GROUPS /
//                                     HANDED: workgroups to re-seed / handed over -> "seeded lean clean drop state"
//       load                          new resident samples -> "loaded"
// A mismatch prints what differed and exits with 1.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "epoch_control.h"

using dbgsom::AnchorControl;
using dbgsom::LeanGate;
using dbgsom::ResidentSearchState;
typedef SearchPolicy::Plan Plan;

namespace {   // (structs that hold the hidden types of the headers)

// ---- what the engine keeps of the resident samples' buckets (Samples: anchor_state, anchor_generation) ----
struct Buckets {
    int state = 0;
    int64_t generation = 0;
    void drop(int s) { state = s; ++generation; }
};

// ---- the parent's fields and text ----
struct Legacy {
    bool hint_valid = false;
    int64_t hintM = 0;
    bool last_idx_valid = false;
    bool dist_bound_valid = false;
    int distW_buf = 0;
    int64_t distW_M = 0;
    int64_t anchor_searches = 0;
    bool anchors_built_now = false;
    bool last_anchor_seeded = false;
    LeanGate lean_gate;
    bool last_lean = false;
    int last_plan_key = 0;
    int64_t lean_searches = 0;
    double prepass_mean = NAN;
    int64_t prepass_M = 0;
};

static void legacy_ensure_anchors(Legacy *c, Buckets &s) {
    if (s.state != 0) return;
    s.state = 1;
    c->anchors_built_now = true;
}

// run_filtered: from `c->last_anchor_seeded = false` to the end of the anchor block -> the call's seed_stride
static int legacy_before_search(Legacy *c, Buckets &s, const Plan &plan, bool prev_idx, bool s_is_xs, int anchor_seeds,
                                int64_t M, bool may_probe) {
    int seed_stride = plan.seed_stride;
    c->last_anchor_seeded = false;
    c->last_lean = false;
    c->last_plan_key = LeanGate::plan_key(plan.seed_stride & ~DBGSOM_PRUNE_RETRY, plan.sweep_planes);
    const bool has_ref = c->prepass_mean == c->prepass_mean && SearchPolicy::near_size(M, c->prepass_M);
    if (!prev_idx && s_is_xs && anchor_seeds && s.state != 2 && has_ref && plan.planes == 0 &&
        !plan.seed_full && (plan.seed_stride & DBGSOM_PRUNE)) {
        legacy_ensure_anchors(c, s);
        ++c->anchor_searches;
        c->last_anchor_seeded = true;
        if (may_probe && c->lean_gate.allows(M, s.generation, c->last_plan_key, plan.retry, plan.refine)) {
            seed_stride |= DBGSOM_ANCHOR_LISTS_ONLY;
            c->last_lean = true;
            ++c->lean_searches;
        }
    }
    return seed_stride;
}

// dbgsom_ctx_epoch: the block behind smooth_and_fetch for a filtered epoch, up to pol.observe -> clean
static bool legacy_after_epoch(Legacy *c, Buckets &s, const SearchPolicy &pol, const double *counted, int64_t N, int64_t M,
                               int measuring, const double *W_new_host, const int64_t *idx_host, const double *dist_host) {
    const bool lean_missed = c->last_lean && counted[3] > 0.0;
    if (c->last_anchor_seeded) c->lean_gate.record(M, s.generation, c->last_plan_key, counted[3], counted[2]);
    else c->lean_gate.forget();
    const bool clean = !pol.last_probed && !pol.last_guarded && measuring < 0 && !W_new_host && !idx_host && !dist_host &&
                       !c->anchors_built_now && !lean_missed;
    const int64_t nb = (N + 127) / 128;
    const bool settled = !(counted[2] > 0.0 && !pol.last_retry) && !lean_missed;
    if (pol.last_probed && !pol.last_hinted && !pol.last_seed_full && settled) {
        c->prepass_mean = counted[1] / (double)nb;
        c->prepass_M = M;
    }
    if (pol.planes_used == 0 && !pol.last_hinted && !pol.last_seed_full && settled) {
        const double mean = counted[0] / (double)nb;
        if (c->last_anchor_seeded) {
            if (mean > 1.25 * c->prepass_mean) s.drop(2);
        } else {
            c->prepass_mean = mean;
            c->prepass_M = M;
        }
    }
    return clean;
}
static void legacy_after_unfiltered_epoch(Legacy *c) { c->lean_gate.forget(); }
static void legacy_begin_epoch(Legacy *c) { c->anchors_built_now = false; }

// one function per site that assigned the search state
static void legacy_epoch_bmu_csr(Legacy *c) {
    c->hint_valid = false;
    c->last_idx_valid = true;
    c->dist_bound_valid = false;
}
static void legacy_epoch_bmu_dense(Legacy *c, int cur, int64_t M) {
    c->hint_valid = false;
    c->last_idx_valid = true;
    c->dist_bound_valid = true; c->distW_buf = cur; c->distW_M = M;
}
static void legacy_metric_epoch_before_search(Legacy *c) {
    c->hint_valid = false;
    c->dist_bound_valid = false;
}
static void legacy_metric_epoch_after_search(Legacy *c) { c->last_idx_valid = true; }
static void legacy_update_before_copies(Legacy *c) {
    c->hint_valid = false;
    c->dist_bound_valid = false;
}
static void legacy_update_after_copies(Legacy *c) { c->last_idx_valid = true; }
static void legacy_epoch_sums_made(Legacy *c, int64_t M) {
    c->hint_valid = true;
    c->hintM = M;
}
static void legacy_epoch_error_tail(Legacy *c) { c->hint_valid = false; }
// (the text at 2d7f700 left last_idx_valid alone: dbgsom_ctx_class_histogram(NULL) and dbgsom_ctx_target_statistics(NULL)
//  behind a dbgsom_ctx_set_hint then folded the caller's seeds as if they were the last epoch's winners -- corrected here
//  and in the header together; tests/test_gpu_call_order.py holds the sequence)
static void legacy_set_hint(Legacy *c, int64_t M) {
    c->hint_valid = true;
    c->dist_bound_valid = false;
    c->last_idx_valid = false;
    c->hintM = M;
}
static void legacy_stage_weights(Legacy *c, int cur) { if (c->distW_buf == cur) c->dist_bound_valid = false; }
static void legacy_set_weights(Legacy *c, int cur) { if (c->distW_buf == cur) c->dist_bound_valid = false; }
static void legacy_write_weight_rows(Legacy *c, int cur) { if (c->distW_buf == cur) c->dist_bound_valid = false; }
static void legacy_node_statistics(Legacy *c) { c->hint_valid = false; }
static void legacy_reset_training_state(Legacy *c) {
    c->hint_valid = c->last_idx_valid = false;
    c->prepass_mean = NAN;
    c->last_anchor_seeded = false;
    c->dist_bound_valid = false;
}
static bool legacy_hint_applies(const Legacy *c, bool takes_hint, int64_t M) { return takes_hint && c->hint_valid && c->hintM <= M; }
static bool legacy_bound_usable(const Legacy *c, bool dist_is_epoch_dist, bool wb_p) {
    return c->dist_bound_valid && dist_is_epoch_dist && wb_p;
}

// ---- the new side of one search, as run_filtered drives it -> the call's seed_stride ----
struct Counters { int64_t anchor_searches = 0, lean_searches = 0; };
static int new_before_search(AnchorControl &a, Counters &n, Buckets &s, const Plan &plan, bool hinted, bool resident,
                             bool option_on, int64_t M, bool may_probe) {
    int seed_stride = plan.seed_stride;
    if (a.wants_anchors(plan, hinted, resident, option_on, s.state, M)) {
        if (s.state == 0) { s.state = 1; a.anchors_built(); }   // (ensure_anchors)
        ++n.anchor_searches;
        if (a.anchor_seeded(plan, M, may_probe, s.generation)) {
            seed_stride |= DBGSOM_ANCHOR_LISTS_ONLY;
            ++n.lean_searches;
        }
    }
    return seed_stride;
}

// ---- comparison ----
static bool same_double(double a, double b) { return (a != a && b != b) || a == b; }
static bool same_gate(const LeanGate &a, const LeanGate &b) {
    // (what forget() leaves behind `known` is never read again before a record())
    return a.known == b.known && (!a.known || (a.M == b.M && a.generation == b.generation && a.plan == b.plan &&
                                               same_double(a.handed, b.handed) && same_double(a.long_lists, b.long_lists)));
}
#define REQUIRE(cond, ...) do { if (!(cond)) { printf("MISMATCH " __VA_ARGS__); printf(" [%s]\n", #cond); exit(1); } } while (0)
static void compare_anchor(const Legacy &l, const Buckets &lb, const AnchorControl &a, const Counters &n, const Buckets &nb,
                           const char *where) {
    REQUIRE(l.anchors_built_now == a.anchors_built_now && l.last_anchor_seeded == a.last_anchor_seeded &&
            l.last_lean == a.last_lean && l.last_plan_key == a.last_plan_key && same_double(l.prepass_mean, a.prepass_mean) &&
            l.prepass_M == a.prepass_M && same_gate(l.lean_gate, a.lean_gate), "%s: fields", where);
    REQUIRE(l.anchor_searches == n.anchor_searches && l.lean_searches == n.lean_searches, "%s: counters", where);
    REQUIRE(lb.state == nb.state && lb.generation == nb.generation, "%s: buckets", where);
}
static void compare_state(const Legacy &l, const ResidentSearchState &s, const char *where) {
    REQUIRE(l.hint_valid == s.hint_valid && l.hintM == s.hintM && l.last_idx_valid == s.last_idx_valid &&
            l.dist_bound_valid == s.dist_bound_valid && l.distW_buf == s.distW_buf && l.distW_M == s.distW_M, "%s: fields", where);
    for (int q = 0; q < 4; ++q) {
        REQUIRE(legacy_hint_applies(&l, q & 1, 130 + (q >> 1)) == s.hint_applies(q & 1, 130 + (q >> 1)), "%s: hint_applies", where);
        REQUIRE(legacy_bound_usable(&l, q & 1, q >> 1) == s.bound_usable(q & 1, q >> 1), "%s: bound_usable", where);
    }
}

// the same gate state on both sides; which: 0 unknown, 1 matches (M, generation 1, plan `key`), 2 .. 6 one thing off
static LeanGate gate_state(int which, int64_t M, int key) {
    LeanGate g;
    if (which) g.record(which == 2 ? M + 1 : M, which == 3 ? 2 : 1, which == 4 ? key ^ 1 : key, which == 5 ? 3.0 : 0.0,
                        which == 6 ? 2.0 : 0.0);
    return g;
}
static void seed_both(Legacy &l, AnchorControl &a, const LeanGate &g, double prepass_mean, int64_t prepass_M, bool seeded,
                      bool lean, bool built, int key) {
    l.lean_gate = a.lean_gate = g;
    l.prepass_mean = a.prepass_mean = prepass_mean;
    l.prepass_M = a.prepass_M = prepass_M;
    l.last_anchor_seeded = a.last_anchor_seeded = seeded;
    l.last_lean = a.last_lean = lean;
    l.anchors_built_now = a.anchors_built_now = built;
    l.last_plan_key = a.last_plan_key = key;
}

static const int64_t M0 = 1024, N0 = 4096;   // 32 workgroups: every mean below is an exact quotient
static const double NB0 = 32.0;

static Plan prune_plan(bool retry, bool refine, bool seed_full, int planes, int flags) {
    Plan p;
    p.planes = planes; p.seed_full = seed_full; p.retry = retry; p.refine = refine;
    p.seed_stride = 4 | flags; p.sweep_planes = planes ? planes : 1;
    return p;
}

// ---- enumerate ----
static int enumerate() {
    long long n_before = 0, n_seeded = 0, n_lean = 0, n_built = 0;
    const double means[2] = {NAN, 10.0};
    const int64_t sizes[4] = {M0, 820, 819, 0};   // 1024 is within a quarter of 820 and not of 819
    for (int bits = 0; bits < 512; ++bits)
        for (int planes = 0; planes < 2; ++planes)
            for (int state = 0; state < 3; ++state)
                for (int mi = 0; mi < 2; ++mi)
                    for (int si = 0; si < 4; ++si)
                        for (int gi = 0; gi < 7; ++gi) {
                            const bool hinted = bits & 1, resident = bits & 2, option_on = bits & 4, seed_full = bits & 8,
                                       retry = bits & 16, refine = bits & 32, may_probe = bits & 64;
                            const int flags = (bits & 128 ? DBGSOM_PRUNE : 0) | (bits & 256 ? DBGSOM_PRUNE_RETRY : 0);
                            const Plan plan = prune_plan(retry, refine, seed_full, planes, flags);
                            const int key = LeanGate::plan_key(plan.seed_stride & ~DBGSOM_PRUNE_RETRY, plan.sweep_planes);
                            Legacy l;
                            AnchorControl a;
                            Counters n;
                            Buckets lb, nb;
                            lb.state = nb.state = state;
                            lb.generation = nb.generation = 1;
                            seed_both(l, a, gate_state(gi, M0, key), means[mi], sizes[si], true, true, false, 77);
                            const int ls = legacy_before_search(&l, lb, plan, hinted, resident, option_on ? 1 : 0, M0, may_probe);
                            const int ns = new_before_search(a, n, nb, plan, hinted, resident, option_on, M0, may_probe);
                            REQUIRE(ls == ns, "before_search: seed_stride");
                            compare_anchor(l, lb, a, n, nb, "before_search");
                            ++n_before;
                            n_seeded += a.last_anchor_seeded; n_lean += a.last_lean; n_built += a.anchors_built_now;
                        }
    long long n_after = 0, n_clean[2] = {0, 0}, n_valve[2] = {0, 0}, n_ref = 0, n_probe_ref = 0, n_missed = 0;
    const double thr = 1.25 * 10.0;
    const double lists[3] = {12.0 * NB0, thr * NB0, nextafter(thr, INFINITY) * NB0};
    static const double w_new = 0.0;
    for (int bits = 0; bits < 512; ++bits)
        for (int planes = 0; planes < 3; ++planes)
            for (int measuring = -1; measuring < 1; ++measuring)
                for (int cb = 0; cb < 4; ++cb)
                    for (int li = 0; li < 3; ++li)
                        for (int mi = 0; mi < 2; ++mi)
                            for (int si = 0; si < 2; ++si)
                                for (int out = 0; out < 5; ++out) {   // none, W', winners, distances, all three
                                    SearchPolicy pol;
                                    pol.last_probed = bits & 1; pol.last_guarded = bits & 2; pol.last_hinted = bits & 4;
                                    pol.last_seed_full = bits & 8; pol.last_retry = bits & 16; pol.planes_used = planes;
                                    const bool seeded = bits & 32, lean = bits & 64, built = bits & 128, known = bits & 256;
                                    const bool o_w = out == 1 || out == 4, o_i = out == 2 || out == 4, o_d = out == 3 || out == 4;
                                    const double counted[4] = {lists[li], 5.0 * NB0, cb & 1 ? 3.0 : 0.0, cb & 2 ? 3.0 : 0.0};
                                    Legacy l;
                                    AnchorControl a;
                                    Counters n;
                                    Buckets lb, nb;
                                    lb.state = nb.state = 1;
                                    lb.generation = nb.generation = 1;
                                    seed_both(l, a, gate_state(known ? 1 : 0, M0, 77), means[mi], si ? 819 : 820, seeded, lean,
                                              built, 77);
                                    const bool lc = legacy_after_epoch(&l, lb, pol, counted, N0, M0, measuring, o_w ? &w_new : nullptr,
                                                                       o_i ? (const int64_t *)&w_new : nullptr, o_d ? &w_new : nullptr);
                                    const AnchorControl::Verdict v =
                                        a.after_filtered_epoch(counted, N0, M0, nb.generation, pol, measuring, o_w || o_i || o_d);
                                    if (v.drop_anchors) nb.drop(2);
                                    REQUIRE(lc == v.clean, "after_filtered_epoch: clean");
                                    compare_anchor(l, lb, a, n, nb, "after_filtered_epoch");
                                    ++n_after;
                                    ++n_clean[v.clean]; ++n_valve[v.drop_anchors];
                                    n_missed += lean && counted[3] > 0.0;
                                    const bool moved = !same_double(a.prepass_mean, means[mi]);
                                    n_ref += moved && a.prepass_mean == lists[li] / NB0;
                                    n_probe_ref += moved && a.prepass_mean == 5.0;
                                    // the valve fires one ulp above 1.25 times the reference and never at or below it
                                    // (a counting-only launch of the same epoch replaces the reference first: by 5)
                                    REQUIRE(!v.drop_anchors || (pol.last_probed ? lists[li] / NB0 > 1.25 * 5.0 : li == 2 && mi == 1),
                                            "the valve fired at or below 1.25");
                                }
    printf("before_search %lld\nanchor_seeded %lld\nlean %lld\nbuilt %lld\n", n_before, n_seeded, n_lean, n_built);
    printf("after_filtered_epoch %lld\nclean_true %lld\nclean_false %lld\nvalve_fired %lld\nvalve_not_fired %lld\n", n_after,
           n_clean[1], n_clean[0], n_valve[1], n_valve[0]);
    printf("reference_taken %lld\nprobe_reference_taken %lld\nlean_missed %lld\n", n_ref, n_probe_ref, n_missed);
    return 0;
}

// ---- sequences ----
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static unsigned rnd(unsigned n) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)((rng_state >> 33) % n);
}

enum { STATE_EVENTS = 16 };
static void state_event(int e, Legacy &l, ResidentSearchState &s) {
    switch (e) {
    case 0: legacy_epoch_bmu_dense(&l, 0, 130); s.dense_search_done(0, 130); break;
    case 1: legacy_epoch_bmu_dense(&l, 1, 131); s.dense_search_done(1, 131); break;
    case 2: legacy_epoch_bmu_csr(&l); s.foreign_search_done(); break;
    case 3: legacy_metric_epoch_before_search(&l); s.foreign_search_begun(); break;   // (a metric epoch whose search failed)
    case 4:                                                                           // (... and one whose search ran)
        legacy_metric_epoch_before_search(&l); s.foreign_search_begun();
        legacy_metric_epoch_after_search(&l); s.foreign_search_done();
        break;
    case 5: legacy_update_before_copies(&l); s.foreign_search_begun(); break;         // (an update whose copies failed)
    case 6:
        legacy_update_before_copies(&l); s.foreign_search_begun();
        legacy_update_after_copies(&l); s.caller_winners_taken();
        break;
    case 7: legacy_epoch_sums_made(&l, 130); s.sums_made(130); break;
    case 8: legacy_epoch_sums_made(&l, 131); s.sums_made(131); break;
    case 9: legacy_epoch_error_tail(&l); s.epoch_failed(); break;
    case 10: legacy_set_hint(&l, 130); s.hint_seeded(130); break;
    case 11: legacy_stage_weights(&l, 0); s.weights_replaced(0); break;
    case 12: legacy_set_weights(&l, 1); s.weights_replaced(1); break;
    case 13: legacy_write_weight_rows(&l, 0); s.weights_replaced(0); break;
    case 14: legacy_node_statistics(&l); s.bucket_order_rewritten(); break;
    default: legacy_reset_training_state(&l); s.reset(); break;
    }
}
static int state_step(int e, Legacy &l, ResidentSearchState &s) {
    state_event(e, l, s);
    compare_state(l, s, "state sequence");
    return 1;
}

enum { ANCHOR_EVENTS = 13 };
struct AnchorWorld {
    Legacy l;
    AnchorControl a;
    Counters n;
    Buckets lb, nb;
    SearchPolicy pol;     // the last_* of the last search's plan, as plan() leaves them
    int64_t M = M0;
    void search(const Plan &plan, bool hinted, bool probed, bool epoch) {
        pol.planes_used = plan.planes; pol.last_seed_full = plan.seed_full; pol.last_retry = plan.retry;
        if (epoch) pol.last_hinted = hinted;
        pol.last_probed = probed;
        const int ls = legacy_before_search(&l, lb, plan, hinted, true, 1, M, epoch);
        const int ns = new_before_search(a, n, nb, plan, hinted, true, true, M, epoch);
        REQUIRE(ls == ns, "anchor sequence: seed_stride");
    }
    void after(double mean, double groups, double handed) {
        const double counted[4] = {mean * NB0, 9.0 * NB0, groups, handed};
        const bool lc = legacy_after_epoch(&l, lb, pol, counted, N0, M, -1, nullptr, nullptr, nullptr);
        const AnchorControl::Verdict v = a.after_filtered_epoch(counted, N0, M, nb.generation, pol, -1, false);
        if (v.drop_anchors) nb.drop(2);
        REQUIRE(lc == v.clean, "anchor sequence: clean");
        pol.last_probed = false;   // (SearchPolicy::observe)
    }
    void step(int e) {
        switch (e) {
        case 0: legacy_begin_epoch(&l); a.begin_epoch(); pol.last_hinted = false; break;
        case 1: search(prune_plan(false, false, false, 0, DBGSOM_PRUNE), false, false, true); break;
        case 2: search(prune_plan(true, false, false, 0, DBGSOM_PRUNE | DBGSOM_PRUNE_RETRY), false, false, true); break;
        case 3: search(prune_plan(false, false, false, 1, DBGSOM_PRUNE_PROBE), false, true, true); break;
        case 4: search(prune_plan(false, false, false, 0, DBGSOM_PRUNE), true, false, true); break;
        case 5: search(prune_plan(false, false, false, 0, DBGSOM_PRUNE), false, false, false); break;   // (resident_bmu, k = 1)
        case 6: after(8.0, 0.0, 0.0); break;
        case 7: after(8.0, 0.0, 3.0); break;
        case 8: after(30.0, 0.0, 0.0); break;
        case 9: after(8.0, 3.0, 0.0); break;
        case 10: legacy_after_unfiltered_epoch(&l); a.after_unfiltered_epoch(); break;
        case 11: lb.drop(0); nb.drop(0); legacy_reset_training_state(&l); a.reset(); break;   // (a load)
        default: M = M == M0 ? M0 + 1 : M0; break;                                           // (a growth step, and back)
        }
        compare_anchor(l, lb, a, n, nb, "anchor sequence");
    }
};

static int sequences() {
    long long state_steps = 0, anchor_steps = 0, seeded = 0, lean = 0, dropped = 0;
    for (int len = 1; len <= 5; ++len) {
        long long count = 1;
        for (int i = 0; i < len; ++i) count *= STATE_EVENTS;
        for (long long code = 0; code < count; ++code) {
            Legacy l;
            ResidentSearchState s;
            long long c = code;
            for (int i = 0; i < len; ++i, c /= STATE_EVENTS) state_steps += state_step((int)(c % STATE_EVENTS), l, s);
        }
        count = 1;
        for (int i = 0; i < len; ++i) count *= ANCHOR_EVENTS;
        for (long long code = 0; code < count; ++code) {
            AnchorWorld w;
            long long c = code;
            for (int i = 0; i < len; ++i, c /= ANCHOR_EVENTS, ++anchor_steps) w.step((int)(c % ANCHOR_EVENTS));
            seeded += w.n.anchor_searches; lean += w.n.lean_searches; dropped += w.nb.state == 2;
        }
    }
    long long random_seeded = 0, random_lean = 0, random_dropped = 0;
    for (int r = 0; r < 4000; ++r) {
        Legacy l;
        ResidentSearchState s;
        for (int i = 0; i < 30; ++i) state_steps += state_step((int)rnd(STATE_EVENTS), l, s);
        AnchorWorld w;
        for (int i = 0; i < 30; ++i, ++anchor_steps) w.step((int)rnd(ANCHOR_EVENTS));
        random_seeded += w.n.anchor_searches; random_lean += w.n.lean_searches; random_dropped += w.nb.state == 2;
    }
    printf("state_steps %lld\nanchor_steps %lld\nanchor_seeded %lld\nlean %lld\ndropped %lld\n", state_steps, anchor_steps,
           seeded, lean, dropped);
    printf("random_anchor_seeded %lld\nrandom_lean %lld\nrandom_dropped %lld\n", random_seeded, random_lean, random_dropped);
    return 0;
}

// ---- scenario: the new structs alone, driven as the engine drives them ----
static int scenario() {
    AnchorControl a;
    Counters n;
    Buckets b;
    char cmd[32];
    while (scanf("%31s", cmd) == 1) {
        if (!strcmp(cmd, "epoch")) {
            long long M;
            double mean, groups, handed;
            if (scanf("%lld %lf %lf %lf", &M, &mean, &groups, &handed) != 4) return 2;
            const Plan plan = prune_plan(false, false, false, 0, DBGSOM_PRUNE);
            SearchPolicy pol;
            pol.planes_used = 0; pol.last_probed = false;
            const Counters before = n;
            a.begin_epoch();
            new_before_search(a, n, b, plan, false, true, true, M, true);
            const double counted[4] = {mean * NB0, 0.0, groups, handed};
            const AnchorControl::Verdict v = a.after_filtered_epoch(counted, N0, M, b.generation, pol, -1, false);
            if (v.drop_anchors) b.drop(2);
            printf("%d %d %d %d %d\n", (int)(n.anchor_searches - before.anchor_searches), (int)(n.lean_searches - before.lean_searches),
                   (int)v.clean, (int)v.drop_anchors, b.state);
        } else if (!strcmp(cmd, "load")) {
            b.drop(0);
            a.reset();
            printf("loaded\n");
        } else {
            return 2;
        }
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "enumerate")) return enumerate();
    if (argc == 2 && !strcmp(argv[1], "sequences")) return sequences();
    if (argc == 2 && !strcmp(argv[1], "scenario")) return scenario();
    return 2;
}
