// The engine-side control of the resident k = 1 search, beside the arm policy (search_policy.h): whether a stateless
// search takes its seeds from the anchor buckets and in which form (AnchorControl: the lean gate, the valve and the
// pre-pass reference they rest on), and what the last search left in HBM for the next one (ResidentSearchState: the
// hint, the winners, the pruning bound).  Host-only and free of HIP, like search_policy.h: plain arguments in, plain
// values out, no clock -- the engine (engine.hip) executes what they say, and tests/epoch_control_check.cpp holds
// every decision against the text it replaced.  Results never depend on AnchorControl; speed does.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/dbgsom_hip.h"
#include "lean_gate.h"
#include "search_policy.h"

namespace dbgsom {

struct __attribute__((visibility("hidden"))) AnchorControl {
    // the lean form of the anchor-seeded search (DBGSOM_ANCHOR_LISTS_ONLY): when an epoch takes it (lean_gate.h),
    // whether the last search did, and the plan of the last search
    LeanGate lean_gate;
    bool last_lean = false;
    int last_plan_key = 0;
    // mean list length of the last pruning epoch the cheap pre-pass seeded, and the map it ran on: what the
    // anchors' lists are held against (after_filtered_epoch)
    double prepass_mean = NAN;
    int64_t prepass_M = 0;
    bool last_anchor_seeded = false;    // the last filtered search took its seeds from the anchors
    bool anchors_built_now = false;     // the running epoch built the buckets: its clock is not the arm's

    void begin_epoch() { anchors_built_now = false; }
    void anchors_built() { anchors_built_now = true; }
    void after_unfiltered_epoch() { lean_gate.forget(); }
    // new resident samples (the gate needs no word: the load has bumped the buckets' generation)
    void reset() { prepass_mean = NAN; last_anchor_seeded = false; }

    // One filtered k = 1 search, of an epoch or not, in two steps: the buckets may have to be built in between.
    // A stateless search of the resident samples (`resident`; `option_on`: "anchor_seeds") in the pruning form with
    // the cheap seeds: the seeds come from the anchor buckets instead of the pre-pass.  Nothing the policy sees
    // changes: it planned a stateless call.  Only once the pre-pass has seeded a pruning epoch (or a counting-only
    // pruning launch) of this sample set on a map about this size: what it left is what the anchors' lists are
    // held against (the valve below), and the policy's own first looks at the arm -- are its cheap seeds poor, does
    // it need the re-seeding passes -- are looks at the pre-pass.
    bool wants_anchors(const SearchPolicy::Plan &plan, bool hinted, bool resident, bool option_on, int anchor_state,
                       int64_t M) {
        last_anchor_seeded = last_lean = false;
        // (without the re-seeding bit: an epoch whose re-seeding passes found nothing to do is evidence for the same
        //  plan without them, which is what the policy plans next; a plan WITH them is never lean)
        last_plan_key = LeanGate::plan_key(plan.seed_stride & ~DBGSOM_PRUNE_RETRY, plan.sweep_planes);
        const bool has_ref = prepass_mean == prepass_mean && SearchPolicy::near_size(M, prepass_M);
        return !hinted && resident && option_on && anchor_state != 2 && has_ref && plan.planes == 0 && !plan.seed_full &&
               (plan.seed_stride & DBGSOM_PRUNE);
    }
    // ... and, the buckets standing (`generation`: theirs -- buckets built on the way replace dropped ones and carry
    // another, that epoch is a full one): lean?  The search of an epoch (`may_probe`) behind an anchor-seeded epoch
    // of the same samples, map size and plan that handed nothing to the per-sample pass: nothing is made for that pass.
    bool anchor_seeded(const SearchPolicy::Plan &plan, int64_t M, bool may_probe, int64_t generation) {
        last_anchor_seeded = true;
        last_lean = may_probe && lean_gate.allows(M, generation, last_plan_key, plan.retry, plan.refine);
        return last_lean;
    }

    // clean: the epoch's wall clock is the arm's, nothing rode along; drop_anchors: the valve -- the pre-pass seeds
    // this sample set again (Samples::drop_anchors(2))
    struct Verdict { bool clean, drop_anchors; };
    // After an epoch through the filter whose counts came back, in front of SearchPolicy::observe (which clears
    // last_probed).  counted: lists, probe, groups to re-seed, handed over (pack_results_kernel), over the workgroups
    // of 128 of N samples; `measuring`: the form of the refinement the epoch timed (-1: none); `outputs_asked`:
    // the caller had results copied to the host.
    Verdict after_filtered_epoch(const double counted[4], int64_t N, int64_t M, int64_t generation, const SearchPolicy &pol,
                                 int measuring, bool outputs_asked) {
        // A lean epoch that kept long lists guessed wrong: what it measured is neither what the anchors' lists
        // cost (the per-sample pass would have shortened them) nor a clock of the arm.  The next one is full.
        const bool lean_missed = last_lean && counted[3] > 0.0;
        if (last_anchor_seeded) lean_gate.record(M, generation, last_plan_key, counted[3], counted[2]);
        else lean_gate.forget();
        // (a clean measurement of the arm: nothing rode along -- see SearchPolicy::arm_ms -- and the epoch did not
        //  build the anchor buckets on the way)
        Verdict v = {!pol.last_probed && !pol.last_guarded && measuring < 0 && !outputs_asked && !anchors_built_now &&
                         !lean_missed,
                     false};
        // The valve of the anchor seeds: their lists against those of the last pruning epoch the cheap pre-pass
        // seeded on a map within a quarter of this size (wants_anchors waits for one).  More than 1.25 times
        // that -- a quarter of the exact stage lost at the most -- and the pre-pass seeds this sample set
        // again.  (An epoch whose long lists the policy is about to re-seed is not what either form costs.)
        const int64_t nb = (N + 127) / 128;
        const bool settled = !(counted[2] > 0.0 && !pol.last_retry) && !lean_missed;
        const bool cheap_seeds = !pol.last_hinted && !pol.last_seed_full;
        if (pol.last_probed && cheap_seeds && settled) {
            // (a counting-only pruning launch beside a sweep: the lists the pre-pass's seeds would have left)
            prepass_mean = counted[1] / (double)nb;
            prepass_M = M;
        }
        if (pol.planes_used == 0 && cheap_seeds && settled) {
            const double mean = counted[0] / (double)nb;
            if (last_anchor_seeded) {   // (wants_anchors took them because a reference exists)
                v.drop_anchors = mean > 1.25 * prepass_mean;
            } else {
                prepass_mean = mean;
                prepass_M = M;
            }
        }
        return v;
    }
};

// What the last search of the resident samples left in HBM, one transition per event.
struct __attribute__((visibility("hidden"))) ResidentSearchState {
    bool hint_valid = false;      // idx[icur] and the bucket order behind it may seed the next search ...
    int64_t hintM = 0;            // ... of a map of at least this many prototypes
    bool last_idx_valid = false;  // idx[icur] holds the winners of the last epoch / partition
    // `dist` holds the exact distances of the resident samples to the rows idx[icur] of Wb[distW_buf]
    // (distW_M rows) as the last epoch's search left them: the hinted pruning bound (filter.hip 2c)
    bool dist_bound_valid = false;
    int distW_buf = 0;
    int64_t distW_M = 0;

    // the Euclidean search of an epoch under Wb[buf] (M rows); the hint is re-established by sums_made
    void dense_search_done(int buf, int64_t M) {
        hint_valid = false; last_idx_valid = dist_bound_valid = true; distW_buf = buf; distW_M = M;
    }
    // winners and distances that are no seeds and no bounds of a Euclidean search (CSR rows, another metric, the
    // caller's own): dropped when the buffers are about to be overwritten, the winners valid once they are there
    void foreign_search_begun() { hint_valid = dist_bound_valid = false; }
    void foreign_search_done() { foreign_search_begun(); last_idx_valid = true; }
    void caller_winners_taken() { foreign_search_done(); }   // (dbgsom_ctx_update)
    // the accumulate step of dbgsom_ctx_epoch has left the bucket order of the winners (M prototypes)
    void sums_made(int64_t M) { hint_valid = true; hintM = M; }
    void epoch_failed() { hint_valid = false; }
    // the caller's seeds and their bucket order are in place (dbgsom_ctx_set_hint): no distances go with them, and
    // idx[icur] now holds seeds, not the winners of an epoch -- what reads "the last epoch's winners" must refuse
    void hint_seeded(int64_t M) { hint_valid = true; hintM = M; dist_bound_valid = last_idx_valid = false; }
    // Wb[buf] was overwritten: if the bound's distances refer to it, it is gone
    void weights_replaced(int buf) { if (distW_buf == buf) dist_bound_valid = false; }
    void bucket_order_rewritten() { hint_valid = false; }   // (dbgsom_ctx_node_statistics)
    void reset() { hint_valid = last_idx_valid = dist_bound_valid = false; }

    // the previous epoch's winners seed a search under M prototypes (`takes_hint`: SearchPolicy::takes_hint)
    bool hint_applies(bool takes_hint, int64_t M) const { return takes_hint && hint_valid && hintM <= M; }
    // the bound serves a search that writes the epoch's own distances while the matrix it refers to is allocated
    bool bound_usable(bool into_epoch_dist, bool matrix_there) const { return dist_bound_valid && into_epoch_dist && matrix_there; }
};

}  // namespace dbgsom
