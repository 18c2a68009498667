// The policy of the filtered BMU search: which form of it runs next, epoch by epoch.  Host-only and free of HIP:
// everything it needs arrives as plain arguments, everything the engine needs comes back as plain values, and it
// never reads a clock (the engine hands it milliseconds) -- so a recorded sequence of calls replays bit for bit on
// any CPU (tests/policy_replay.cpp, tests/test_search_policy_cpu.py).  Results never depend on any of this; speed
// does.  The engine (engine.hip) keeps one SearchPolicy per context and executes what it says.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/dbgsom_hip.h"

// (hidden: the inline members of a header-only struct must not join the exported symbols of the library)
struct __attribute__((visibility("hidden"))) SearchPolicy {
    // ---- the cost model and its limits (mirrored by hand in dbgsom_amd/backend.py; the mirror is checked by
    //      tests/test_search_policy_cpu.py) ----
    static constexpr int64_t FILTER_MIN_PROTOTYPES = 129;  // at or below 128 one chunk of the all-pairs kernel is cheaper (measured)
    static constexpr int64_t FILTER_MAX_FEATURES = 43690;  // int32 digit-product accumulators: 3 x 128 x 128 x d < 2^31
    static constexpr int FILTER_BACKOFF = 8;
    // epochs an arm is kept before its alternatives get another look: a map in training changes (early,
    // nearly collapsed maps want a fine sweep, organised ones the coarse one), and only running an arm
    // tells how long its lists are; a look costs one epoch of an arm that could at best be cheaper
    static constexpr int PLANES_REPROBE = 16;
    // cost model of the candidate sweep (per prototype, in units of the three-product sweep) against a
    // list entry of the exact stage -- measured at C4 with this build's kernels: one product 1.00 ms,
    // three 2.87 ms per 1024 prototypes; exact stage 1.16 ms per 33 list entries
    static constexpr double SWEEP_COST[4] = {0.0, 0.35, 1.0, 1.96};
    static constexpr double LIST_COST = 12.5;
    // arm 0 of the policy: no sweep, candidates from the triangle inequality (filter.hip 2c).  In the same
    // units: one pass over the X plane ~ 170 prototypes of the one-product sweep (C4: 0.17 of 1.0 ms per
    // 1024), plus the M x M gap matrix (three products, a third of the sweep's rate: ~ 9 M / N sweeps)
    static constexpr double PRUNE_PASS_COST = 60.0;
    static constexpr int64_t PRUNE_MAX_M = 8192;
    static constexpr double SEED_COST[3] = {1.15, 2.0, 1.0};
    // prior of the per-sample refinement (what has not been measured is not tried blind): the refinement reads two
    // digit planes and the rows once more whatever the lists are -- short lists, few features or a few workgroups
    // never pay; lists beyond twice its largest tile stay the matrix-core stage's anyway
    static constexpr double REFINE_MIN_LISTS = 24.0, REFINE_MAX_LISTS = 400.0;
    static constexpr int64_t REFINE_MIN_FEATURES = 256, REFINE_MIN_ROWS = 65536;

    // ---- options ----
    int algorithm = DBGSOM_ALG_AUTO;
    int sweep_planes = 0;
    int seed_stride = 0;
    // per-sample refinement in front of the exact stage (filter.hip 2d): 0 = off, 1 = on, 2 = by measurement
    // (per arm of the search policy, once it has settled on the arm: the first training epochs are timed with and
    // without it -- wall clock of the whole blocking epoch call, best of two -- and the faster form kept;
    // measured again when the arm's lists change by a quarter)
    int refine = 2;
    int64_t max_mean_candidates = 320;

    // ---- the refinement measurement ----
    struct RefineTimes {
        double ms[2] = {NAN, NAN};  // epoch without / with the refinement: best of two
        int n[2] = {0, 0};
        double mean_ref = NAN;      // the lists these were measured on
    };
    RefineTimes rf[12];             // [4 seeds + planes]
    int rf_arm = 0;                 // the arm of the running call
    int64_t rf_M = -1;
    int rf_measuring = -1;          // the form the running call is timing (-1: none)

    // ---- the arms ----
    int filter_backoff = 0, filter_fail = 0;
    int planes_next = 1, planes_used = 1;   // 1 .. 3 digit planes of the sweep; 0 = no sweep (triangle pruning)
    bool probe_next = false, last_probed = false;  // a counting-only pruning launch beside the sweep
    bool last_retry = false;
    bool exploring_next = false;   // the next epoch runs an arm that has never run on this map (adapt_arms)
    bool last_guarded = false;     // the last filtered search stopped at its lists and ran all pairs instead
    int64_t guarded_calls = 0;
    bool prune_retry = false;  // the last pruning launch met workgroups with poor seeds: re-seed those (DBGSOM_PRUNE_RETRY)
    double last_probe_mean = NAN;
    int64_t planeM = -1;
    double arm_known[3][4] = {{NAN, NAN, NAN, NAN}, {NAN, NAN, NAN, NAN}, {NAN, NAN, NAN, NAN}};  // [seeds][planes]
    double arm_seen[3][4] = {{NAN, NAN, NAN, NAN}, {NAN, NAN, NAN, NAN}, {NAN, NAN, NAN, NAN}};   // last result ever
    int arm_age[3][4] = {};   // updates of the map since the arm last ran
    // measured: wall clock (ms) of the blocking epoch call when the arm last ran WITHOUT anything riding along (a
    // counting-only launch, the refinement's own measurements, results copied to the host).  The re-seeding passes
    // of the pruning arm are NOT "riding along": `prune_retry` stays on for as long as the arm's cheap seeds leave
    // workgroups with long lists, so they are what the arm costs on this data (round 3's advisor asked to drop such
    // epochs: with the flag sticky no arm would ever be timed again -- tests/test_gpu_parity.py
    // test_search_arms_that_have_been_timed_...); sweep arms do not look at the flag at all.
    // two arms that both have one are compared by it, the cost model only prices arms that have none
    double arm_ms[3][4] = {{NAN, NAN, NAN, NAN}, {NAN, NAN, NAN, NAN}, {NAN, NAN, NAN, NAN}};
    double last_epoch_ms = NAN;     // of the epoch observe() is looking at (NaN: not a clean measurement)
    int arm_duels[3][4] = {};       // clean epochs an arm was given only to be timed
    int arm_wait[3][4] = {{16, 16, 16, 16}, {16, 16, 16, 16}, {16, 16, 16, 16}};
    bool last_frozen = false;
    int plane_hold = 0;
    int seed_mode = 0;   // stateless seeds: 0 = the cheap pre-pass, 1 = the full one
    double best_mean = NAN;  // list length of the cheapest known arm (what the back-off looks at)
    bool last_seed_full = false;
    bool last_hinted = false;
    double last_mean = NAN;
    int64_t last_M = 0;      // prototypes of the last filtered k = 1 search

    // what one filtered k = 1 search runs
    struct Plan {
        int planes = 1;                 // 1 .. 3 digit planes, 0 = triangle pruning
        bool seed_full = false;         // the full stateless pre-pass
        bool probe = false;             // a counting-only pruning launch beside the sweep
        bool retry = false;             // re-seed workgroups whose cheap seeds missed (DBGSOM_PRUNE_RETRY)
        bool hint_bound = false;        // hand the call the last epoch's distances and the prototypes' shifts
        int seed_stride = 0, sweep_planes = 1;   // the two arguments of dbgsom_bmu_filtered
        bool refine = false;
        int refine_rows = 0;            // FilteredCall::refine_rows
        int timing_form = -1;           // the form of the refinement this epoch times (-1: none)
        double guard_mean = 0.0;        // FilteredCall::guard_mean
    };

    // The mean list length `auto` bears before it goes back to the all-pairs kernel: the option (320), and never more
    // than half the map -- in the cost model's units an arm costs (its sweep) x M + 12.5 x (mean list) against the
    // all-pairs kernel's 8.4 x M, so lists beyond ~0.5 .. 0.65 M lose to it whatever the arm.  (A young, still collapsed
    // map of a growing fit: at M = 130 .. 260 the lists were 0.75 M and a filtered epoch cost 8 .. 14 ms against 6 .. 7
    // of all pairs -- profiles/r04_fit_trace_before.txt.)
    double bearable_mean(int64_t M) const { return fmin((double)max_mean_candidates, 0.5 * (double)M); }

    // the shapes the filtered search takes at all
    static bool shape_ok(int64_t M, int64_t N, int64_t dp) {
        return M >= FILTER_MIN_PROTOTYPES && M <= DBGSOM_MAX_PROTOTYPES && dp <= FILTER_MAX_FEATURES && N >= 1;
    }
    // the options' and the back-off's say on whether a search of the resident samples goes through the filter
    bool filter_allowed() const {
        if (algorithm == DBGSOM_ALG_EXACT) return false;
        return !(algorithm == DBGSOM_ALG_AUTO && filter_backoff > 0);
    }
    // seeds = the previous epoch's winners whenever the algorithm allows them and they exist
    bool takes_hint() const { return algorithm == DBGSOM_ALG_AUTO || algorithm == DBGSOM_ALG_FILTERED_HINT; }

    // what the next filtered search runs: 1 .. 3 digit planes, 0 = triangle pruning (option value 4)
    int planes_for_call() const { return sweep_planes ? (sweep_planes == 4 ? 0 : sweep_planes) : planes_next; }
    // the (seed_stride, sweep_planes) arguments of dbgsom_bmu_filtered for arm `planes`
    static void call_args(int planes, bool probe, bool retry, int64_t M, int *stride, int *planes_arg) {
        *planes_arg = planes ? planes : 1;
        if (!planes && M <= PRUNE_MAX_M) *stride |= DBGSOM_PRUNE | (retry ? DBGSOM_PRUNE_RETRY : 0);
        else if (probe && M <= PRUNE_MAX_M) *stride |= DBGSOM_PRUNE_PROBE | (retry ? DBGSOM_PRUNE_RETRY : 0);
    }
    // ... of a one-off query batch (stateless, nothing is learnt from it)
    void query_args(int64_t M, int *stride, int *planes_arg) const {
        *stride = seed_stride;
        call_args(planes_for_call(), false, prune_retry, M, stride, planes_arg);
    }

    // k = 2 (topographic error) goes through the pruning form of the filtered search when the training epochs have
    // shown that it works on this data -- arm 0 of the policy has run (or been counted) on this map size and left
    // lists a fraction of the map (clustered data); otherwise all pairs.  NaN: nothing known.
    double k2_lists(int64_t M) const {
        double lists0 = NAN;
        if (planeM == M)
            for (int r = 0; r < 3; ++r) {
                const double v = arm_seen[r][0];
                if (v == v && !(lists0 <= v)) lists0 = v;
            }
        return lists0;
    }
    bool k2_prunes(int64_t M) const {
        const double lists0 = k2_lists(M);
        return M <= PRUNE_MAX_M && M >= 2 && last_M == M && lists0 == lists0 && lists0 <= bearable_mean(M);
    }
    int k2_seed_stride(bool hinted) const {
        return seed_stride | DBGSOM_PRUNE | (prune_retry && !hinted ? DBGSOM_PRUNE_RETRY : 0);
    }

    void set_refine(int v) {
        refine = v;
        for (auto &r : rf) r = RefineTimes();
    }

    // new resident samples: what was learnt on the old ones is gone.  (Field by field what a load has always reset:
    // the arm tables go with planeM at the next observe(); the diagnostic counters and the last_* flags of the last
    // call stay.)
    void reset() {
        filter_backoff = filter_fail = 0;
        planes_next = 1;
        planeM = -1;
        plane_hold = 0;
        seed_mode = 0;
        probe_next = last_probed = false;
        prune_retry = false;
        last_mean = NAN;
        rf_M = -1;
        for (auto &r : rf) r = RefineTimes();
    }

    // a map within a quarter of the size something was learnt on (a growth step: see adapt_arms)
    static bool near_size(int64_t M, int64_t ref) {
        const long long apart = M > ref ? (long long)(M - ref) : (long long)(ref - M);
        return apart * 4 <= (long long)ref;
    }

    void begin_epoch() { last_hinted = false; }

    // One k = 1 search of N rows of dp (padded) features under M prototypes through the filter.  `hinted`: the
    // previous winners seed it; `training`: the search of an epoch (its lists come back through observe());
    // `bound_usable`: the exact distances of the last epoch's winners are still around.
    Plan plan(int64_t M, int64_t N, int64_t dp, bool hinted, bool training, bool bound_usable) {
        Plan pl;
        planes_used = planes_for_call();
        if (planes_used == 0 && M > PRUNE_MAX_M) planes_used = 1;
        last_seed_full = !hinted && seed_mode == 1 && seed_stride == 0;
        if (training) last_hinted = hinted;
        int stride = last_seed_full ? DBGSOM_SEED_FULL : seed_stride, planes_arg = 1;
        // (a probe is read by the policy after a training epoch; the first epoch of a map size always has one)
        last_probed = training && sweep_planes == 0 && (probe_next || planeM != M) && planes_used != 0 && M <= PRUNE_MAX_M;
        if (training) probe_next = false;
        // seeds = the last epoch's winners, and their exact distances are still around: the pruning
        // bound need not read X for samples whose prototype has hardly moved
        pl.hint_bound = training && hinted && bound_usable && M <= PRUNE_MAX_M && (planes_used == 0 || last_probed);
        last_retry = prune_retry;
        call_args(planes_used, last_probed, prune_retry, M, &stride, &planes_arg);
        pl.planes = planes_used; pl.seed_full = last_seed_full; pl.probe = last_probed; pl.retry = last_retry;
        pl.seed_stride = stride; pl.sweep_planes = planes_arg;
        // the tile of the refinement's first list-length class: what the lists were last time, with some room
        // (longer lists go to its largest tile, beyond that to the matrix-core stage)
        int rf_rows = 64;
        const bool mean_known = last_mean == last_mean && last_M == M;
        if (mean_known) rf_rows = (int)(last_mean * 1.25 + 8.0);
        bool use_refine = refine == 1;
        rf_measuring = -1;
        rf_arm = 4 * (hinted ? 2 : (last_seed_full ? 1 : 0)) + planes_used;
        if (refine == 2 && mean_known) {
            if (rf_M > 0 && near_size(M, rf_M)) rf_M = M;   // (a growth step: see adapt_arms)
            if (rf_M != M) {
                rf_M = M;
                for (auto &r : rf) r = RefineTimes();
            }
            RefineTimes &r = rf[rf_arm];
            // (the lists of THIS arm: what it left the last time it ran, else what the last epoch had)
            const double arm_mean = arm_known[rf_arm >> 2][rf_arm & 3];
            const double lists = arm_mean == arm_mean ? arm_mean : last_mean;
            if (!(fabs(lists - r.mean_ref) <= 0.25 * r.mean_ref)) { r = RefineTimes(); r.mean_ref = lists; }
            const bool eligible = lists >= REFINE_MIN_LISTS && lists <= REFINE_MAX_LISTS && dp >= REFINE_MIN_FEATURES &&
                                  N >= REFINE_MIN_ROWS;
            // timed only on an arm the policy has settled on (or the caller fixed): two forms of the SAME search
            const bool settled = sweep_planes != 0 || plane_hold > 0;
            if (!eligible) use_refine = false;
            else if (training && settled && r.n[0] < 2) { use_refine = false; rf_measuring = 0; }
            else if (training && settled && r.n[1] < 2) { use_refine = true; rf_measuring = 1; }
            else use_refine = r.n[0] >= 2 && r.n[1] >= 2 && r.ms[1] < r.ms[0];
        }
        pl.refine = use_refine;
        pl.refine_rows = use_refine ? rf_rows : 0;
        pl.timing_form = rf_measuring;
        // An arm on trial (`auto`, a training epoch, nothing known of this arm on this map): the call stops at lists
        // that average more than the policy bears and the all-pairs kernel finds the winners instead -- the policy
        // still learns what the arm leaves, for the price of its sweep instead of an exact stage over the whole map.
        last_guarded = false;
        const int arm_row = hinted ? 2 : (last_seed_full ? 1 : 0);
        if (training && algorithm == DBGSOM_ALG_AUTO && (planeM != M || isnan(arm_seen[arm_row][planes_used])))
            pl.guard_mean = bearable_mean(M);
        last_M = M;
        return pl;
    }

    // the call stopped at its lists (DBGSOM_LISTS_LONG) and all pairs ran instead
    void on_guarded() {
        last_guarded = true;
        ++guarded_calls;
        rf_measuring = -1;
    }

    // an epoch of `auto` that ran all pairs: the back-off counts down
    void on_exact_epoch() { if (filter_backoff > 0) --filter_backoff; }

    // the form of the refinement the running epoch times (-1: none); asked once per epoch
    int take_timing_form() {
        const int measuring = rf_measuring;
        rf_measuring = -1;
        return measuring;
    }
    // wall clock of the blocking call behind the upload of W: BMU + sums + smoothing
    void refine_timed(int form, double ms) {
        RefineTimes &r = rf[rf_arm];
        r.ms[form] = r.n[form] == 0 ? ms : fmin(ms, r.ms[form]);
        ++r.n[form];
    }

    // an epoch that went past the filter: there are no lists to look at
    void observe_unfiltered() { last_mean = NAN; }

    // after an epoch through the filter has completed: look at how long the candidate lists were, decide what comes
    // next.  list_sum / probe_sum / retry_groups: what the call counted over its `nb` workgroups of 128 samples;
    // `epoch_ms`: wall clock of the epoch when nothing rode along, else NaN.
    void observe(double list_sum, double probe_sum, double retry_groups, int64_t nb, int64_t M, int64_t dp, bool frozen,
                 double epoch_ms) {
        last_frozen = frozen;
        last_epoch_ms = epoch_ms;
        // Workgroups of the pruning form whose lists came out long (poor cheap seeds) while the re-seeding
        // passes were off: what this call measured of arm 0 is not what the arm costs.  Turn them on and
        // measure again -- the same arm once more, or another counting-only launch.
        bool again = false;
        if (planes_used == 0 || last_probed) {
            const bool need = retry_groups > 0.0;
            if (need && !last_retry && !last_hinted && !last_seed_full) {   // (cheap seeds: re-seeding can help)
                prune_retry = true;
                if (planes_used == 0) {
                    last_mean = nb ? list_sum / (double)nb : 0.0;
                    return;
                }
                last_probed = false;
                again = true;
            } else if (!last_hinted && !last_seed_full) {
                prune_retry = need;
            }
        }
        const double mean = nb ? list_sum / (double)nb : 0.0;
        last_mean = mean;
        last_probe_mean = last_probed && nb ? probe_sum / (double)nb : NAN;
        adapt_arms(mean, M, nb * 128, dp);
        if (again) probe_next = true;
        if (algorithm == DBGSOM_ALG_AUTO) {
            // (the cheapest arm known so far, not an arm that is only being looked at)
            // (not while an arm that has never run on this map is up next: on unclustered data the strong corner --
            //  good seeds and a finer sweep -- is what works, and eight all-pairs epochs in front of its first try
            //  cost forty settled ones)
            if (best_mean > bearable_mean(M) && !exploring_next) {  // exponential back-off, capped
                filter_fail = filter_fail < 6 ? filter_fail + 1 : 6;
                filter_backoff = FILTER_BACKOFF << (filter_fail - 1);
            } else if (best_mean > bearable_mean(M)) {
                // (exploring)
            } else {
                filter_fail = 0;
            }
        }
    }

    // what the cost model charges an arm apart from its lists
    // (arm 0: the one-product pre-pass, one pass over the X plane and the gap matrix)
    static double fixed_cost(int s_, int q, int64_t M, int64_t N, int64_t dp) {
        if (q == 0)  // (+ two short dependent launches, ~25 us: what decides on small sample sets)
            return (SEED_COST[s_] - 1.0) * SWEEP_COST[1] * (double)M + PRUNE_PASS_COST +
                   SWEEP_COST[1] * (double)M * 9.0 * (double)M / (double)(N > 0 ? N : 1) +
                   25.0 / (2.8 * ((double)(N > 0 ? N : 1) * (double)dp) / (1.0e6 * 784.0));
        return SEED_COST[s_] * SWEEP_COST[q] * (double)M;
    }
    // ... and an arm that has never been timed as a whole
    static double model_cost(int s_, int q, double lists, int64_t M, int64_t N, int64_t dp) {
        return fixed_cost(s_, q, M, N, dp) + LIST_COST * lists;
    }

    // What the next filtered search runs: an ARM = (seeds, digit planes).  Seeds: 0 = the cheap stateless
    // pre-pass (every 4th .. 64th prototype on three 64-feature blocks), 1 = the full one (every
    // prototype, every feature: one more sweep), 2 = the previous epoch's winners (not a choice: whenever
    // the caller's algorithm allows them and they exist).  Digit planes 1 .. 3 of the candidate sweep.
    // Cost model per arm: seeds {1.15, 2, 1} x SWEEP_COST[planes] x M + LIST_COST x mean list length.
    // The lists of an arm are only known once it has run, so the policy explores: from the cheapest
    // known arm it tries an unknown arm when even EMPTY lists would make it cheaper -- its neighbours
    // (one coordinate changed) first, and, when the lists are long (weakly clustered data: a seed that
    // is not nearly the winner, or a bound as wide as the spread of the distances, leaves most of the
    // map a candidate), the strong corner (full seeds, three products) directly: on isotropic data no
    // single step leads there (full seeds alone: 1024 candidates, finer planes alone: 981, both: 17).
    // When nothing is left to try it stays for PLANES_REPROBE epochs, then forgets the alternatives.
    // Results never depend on any of this.
    void adapt_arms(double mean, int64_t M, int64_t N, int64_t dp) {
        exploring_next = false;
        const int row = last_hinted ? 2 : (last_seed_full ? 1 : 0);
        const int p = planes_used;
        // A growing map changes its size by a few neurons at a time: what the arms left on a map within a quarter of
        // this one's size stays the best guess there is (lists and times move with it by a few per cent, and every arm
        // is looked at again as it ages) -- forgetting it at every growth step made every step pay for the
        // exploration again, on unclustered data an epoch or two at ten times the settled cost.
        if (planeM > 0 && planeM != M && near_size(M, planeM)) planeM = M;
        if (planeM != M) {  // another map size: what was learnt no longer applies
            planeM = M;
            for (auto &r : arm_known) for (double &k : r) k = NAN;
            for (auto &r : arm_seen) for (double &k : r) k = NAN;
            for (auto &r : arm_ms) for (double &k : r) k = NAN;
            for (auto &r : arm_duels) for (int &k : r) k = 0;
            for (auto &r : arm_wait) for (int &k : r) k = 16;
            plane_hold = 0;
        }
        auto fixed = [&](int s_, int q) { return fixed_cost(s_, q, M, N, dp); };
        // an arm's age = how often the map has been UPDATED since it ran (a frozen map -- the bench, a
        // series of queries -- does not age what is known about it)
        if (!last_frozen)
            for (auto &r : arm_age) for (int &a : r) ++a;
        const bool remeasured = !isnan(arm_seen[row][p]);
        arm_known[row][p] = arm_seen[row][p] = mean;
        arm_age[row][p] = 0;
        // (an arm that left more than the policy bears gets its next look late: a look at it costs an all-pairs epoch)
        if (mean > bearable_mean(M)) arm_wait[row][p] = 128;
        if (!isnan(last_epoch_ms))   // (the mean of the last two looks: one epoch's clock jitters by a few per cent)
            arm_ms[row][p] = isnan(arm_ms[row][p]) ? last_epoch_ms : 0.5 * (arm_ms[row][p] + last_epoch_ms);
        if (last_probed) {  // what arm 0 would have produced from the same seeds
            arm_known[row][0] = arm_seen[row][0] = last_probe_mean;
            arm_age[row][0] = 0;
        }
        auto allowed = [&](int s_, int q) {
            if (sweep_planes && q != (sweep_planes == 4 ? 0 : sweep_planes)) return false;  // fixed by the caller
            if (q == 0 && M > PRUNE_MAX_M) return false;
            if (row == 2) return s_ == 2;                                      // hinted: only the planes vary
            return s_ == 0 || (s_ == 1 && seed_stride == 0);               // a caller's stride: cheap seeds only
        };
        if (plane_hold > 0) {
            best_mean = mean;
            // A contender the model prices within a factor of two of this arm and that has never run clean: one epoch
            // of it, on its own, and the clock decides between the two (once per arm until it ages out).
            if (!isnan(arm_ms[row][p])) {
                int ds = -1, dq = -1;
                double dc = 2.0 * (fixed(row, p) + LIST_COST * mean);
                for (int s_ = 0; s_ < 3; ++s_)
                    for (int q = 0; q <= 3; ++q)
                        if (allowed(s_, q) && !(s_ == row && q == p) && !isnan(arm_known[s_][q]) &&
                            isnan(arm_ms[s_][q]) && arm_duels[s_][q] < 1) {
                            const double cst = fixed(s_, q) + LIST_COST * arm_known[s_][q];
                            if (cst < dc) { dc = cst; ds = s_; dq = q; }
                        }
                if (ds >= 0) {
                    ++arm_duels[ds][dq];
                    seed_mode = ds == 1 ? 1 : 0;
                    planes_next = dq;
                    plane_hold = 0;
                    exploring_next = true;
                    return;
                }
            }
            if (--plane_hold == 0) {
                // The alternatives get another look once the map has moved on: an arm whose sweep /
                // pre-pass costs LESS than the current one after arm_wait (16, doubling up to 128 every
                // time the look does not pay) updates of the map -- one epoch that can only be dearer by
                // its lists; a dearer arm after 128 (a look at the full pre-pass is a whole extra sweep).
                for (int s_ = 0; s_ < 3; ++s_)
                    for (int q = 0; q <= 3; ++q) {
                        if ((s_ == row && q == p) || isnan(arm_known[s_][q])) continue;
                        const int wait = fixed(s_, q) < fixed(row, p) ? arm_wait[s_][q] : 128;
                        if (arm_age[s_][q] >= wait) { arm_known[s_][q] = arm_ms[s_][q] = NAN; arm_duels[s_][q] = 0; }
                    }
            }
            return;
        }
        // An arm that has been timed costs what it took; the model prices the others.  Both in the model's units: the
        // timed arms give the units per millisecond (geometric mean of model cost / time over them).
        double log_sum = 0.0;
        int n_timed = 0;
        for (int s_ = 0; s_ < 3; ++s_)
            for (int q = 0; q <= 3; ++q)
                if (!isnan(arm_known[s_][q]) && arm_ms[s_][q] > 0.0) {
                    log_sum += log((fixed(s_, q) + LIST_COST * arm_known[s_][q]) / arm_ms[s_][q]);
                    ++n_timed;
                }
        const double per_ms = n_timed ? exp(log_sum / n_timed) : NAN;
        auto priced = [&](int s_, int q, double lists) {
            return arm_ms[s_][q] > 0.0 ? arm_ms[s_][q] * per_ms : fixed(s_, q) + LIST_COST * lists;
        };
        int bs = row, bp = p;
        double bc = priced(row, p, mean);
        for (int s_ = 0; s_ < 3; ++s_)
            for (int q = 0; q <= 3; ++q)
                if (allowed(s_, q) && !isnan(arm_known[s_][q]) && !(s_ == row && q == p)) {
                    const double cst = priced(s_, q, arm_known[s_][q]);
                    if (cst < bc) { bc = cst; bs = s_; bp = q; }
                }
        // unknown arms worth a look, cheapest optimistic cost first
        int es = -1, ep = -1;
        double ec = bc;
        auto consider = [&](int s_, int q) {
            if (s_ < 0 || s_ > 2 || q < 0 || q > 3 || !allowed(s_, q) || !isnan(arm_known[s_][q])) return;
            // (no list is cheaper than one step of the exact stage: 16 entries)
            const double opt = fixed(s_, q) + LIST_COST * fmin(16.0, (double)M);
            if (opt < ec) { ec = opt; es = s_; ep = q; }
        };
        const double best = (bs == row && bp == p) ? mean : arm_known[bs][bp];
        best_mean = best;
        if (best > fmax(96.0, (double)M / 8.0)) {   // long lists: the strong corner first
            consider(bs == 2 ? 2 : 1, 2);
            if (es < 0) consider(bs == 2 ? 2 : 1, 3);
        }
        if (es < 0) {
            consider(bs, 0);  // (never run blind: see below)
            consider(bs, bp + 1); consider(bs, bp - 1);
            if (bs != 2) consider(1 - bs, bp);
        }
        // arm 0 is looked at by a counting-only launch beside an arm whose lists are known to be
        // bearable (isotropic data: the whole map survives the triangle inequality -- an exact stage
        // over such lists would cost ten ordinary epochs)
        // (the launch counts from the seeds of the call it rides on: that call uses the seeds of the arm
        //  being looked at, with a sweep whose cost is known or about to be)
        if (es >= 0 && ep == 0) {
            probe_next = true;
            ep = bp ? bp : 1;
        }
        if (remeasured)  // a second look at this arm: did it pay?
            arm_wait[row][p] = (bs == row && bp == p) ? 16 : (arm_wait[row][p] >= 64 ? 128 : 2 * arm_wait[row][p]);
        if (es >= 0) {
            seed_mode = es == 1 ? 1 : 0;
            planes_next = ep;
            exploring_next = true;
        } else {
            seed_mode = bs == 1 ? 1 : 0;
            planes_next = bp;
            plane_hold = PLANES_REPROBE;
        }
    }
};
