// Replays a trace of calls into the search policy (dbgsom_amd/csrc/search_policy.h) on the CPU: one step per line on
// stdin, one line of output after every step that returns or changes something a caller can see.  Doubles are
// printed with %a, so two runs agree exactly or not at all (tests/test_search_policy_cpu.py compares strings).
//
//   opt NAME VALUE                   algorithm | sweep_planes | seed_stride | refine | max_mean_candidates
//   reset                            new resident samples
//   shape M N DP                     prototypes, resident rows and padded features of the steps that follow
//   allowed                       -> a  <0|1>                 does a search of this shape go through the filter?
//   plan HINTED TRAINING BOUND    -> p  planes seed_full probe retry hint_bound seed_stride sweep_planes refine
//                                       refine_rows timing_form guard_mean, and the `hinted` the diagnostics now show
//   guarded                          the planned call stopped at its lists
//   refine_timed FORM MS             the epoch timed this form of the refinement
//   observe LIST_SUM PROBE_SUM RETRY_GROUPS FROZEN EPOCH_MS
//                                 -> s  (the state line, see print_state); the sums are over (N + 127) / 128 groups
//   exact_epoch [COUNT]           -> s  COUNT (1) epochs that ran all pairs
//   k2 HINTED                     -> k  <0|1> seed_stride     the k = 2 search of the resident samples
//   query                         -> q  seed_stride sweep_planes      a one-off query batch of M prototypes
//   cost SEEDS PLANES LISTS       -> c  what the cost model charges an arm that has never been timed
// A training plan is preceded by begin_epoch(), as in the engine.  `--constants` prints the cost model instead.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "search_policy.h"

namespace {

// FNV-1a over everything the policy keeps that the state line does not spell out: a difference in any of it shows
// at the step where it arises, not epochs later when a decision finally flips
struct Hash {
    uint64_t h = 1469598103934665603ull;
    void bytes(const void *p, size_t n) {
        for (size_t i = 0; i < n; ++i) { h ^= ((const unsigned char *)p)[i]; h *= 1099511628211ull; }
    }
    void f(double v) {
        if (v != v) v = NAN;   // (one NaN)
        if (v == 0.0) v = 0.0; // (one zero)
        bytes(&v, sizeof v);
    }
    void i(int64_t v) { bytes(&v, sizeof v); }
};

void print_state(const SearchPolicy &p) {
    Hash h;
    for (int s = 0; s < 3; ++s)
        for (int q = 0; q < 4; ++q) {
            h.f(p.arm_known[s][q]); h.f(p.arm_seen[s][q]); h.f(p.arm_ms[s][q]);
            h.i(p.arm_age[s][q]); h.i(p.arm_duels[s][q]); h.i(p.arm_wait[s][q]);
        }
    for (const auto &r : p.rf) { h.f(r.ms[0]); h.f(r.ms[1]); h.i(r.n[0]); h.i(r.n[1]); h.f(r.mean_ref); }
    h.i(p.rf_M); h.i(p.rf_arm); h.i(p.rf_measuring); h.i(p.planeM); h.i(p.last_M); h.i(p.guarded_calls);
    h.i(p.last_retry); h.i(p.last_guarded); h.i(p.last_frozen); h.f(p.last_epoch_ms); h.i(p.filter_fail);
    h.i(p.exploring_next); h.f(p.best_mean);
    const int row = p.last_hinted ? 2 : (p.last_seed_full ? 1 : 0);
    // planes_used planes_next seed_mode prune_retry plane_hold filter_backoff probe_next, hinted seed_full probed,
    // last_mean last_probe_mean, ms of the arm that ran, hash of the rest
    printf("s %d %d %d %d %d %d %d %d %d %d %a %a %a %016llx\n", p.planes_used, p.planes_for_call(), p.seed_mode,
           (int)p.prune_retry, p.plane_hold, p.filter_backoff, (int)p.probe_next, (int)p.last_hinted, (int)p.last_seed_full,
           (int)p.last_probed, p.last_mean, p.last_probe_mean, p.arm_ms[row][p.planes_used], (unsigned long long)h.h);
}

int constants() {
    SearchPolicy p;
    printf("FILTER_MIN_PROTOTYPES %lld\n", (long long)SearchPolicy::FILTER_MIN_PROTOTYPES);
    printf("FILTER_MAX_FEATURES %lld\n", (long long)SearchPolicy::FILTER_MAX_FEATURES);
    printf("MAX_PROTOTYPES %lld\n", (long long)DBGSOM_MAX_PROTOTYPES);
    printf("FILTER_MAX_MEAN_CANDIDATES %lld\n", (long long)p.max_mean_candidates);
    printf("FILTER_BACKOFF %d\n", SearchPolicy::FILTER_BACKOFF);
    printf("PLANES_REPROBE %d\n", SearchPolicy::PLANES_REPROBE);
    printf("PRUNE_MAX_M %lld\n", (long long)SearchPolicy::PRUNE_MAX_M);
    for (int q = 1; q <= 3; ++q) printf("SWEEP_COST_%d %a\n", q, SearchPolicy::SWEEP_COST[q]);
    for (int s = 0; s < 3; ++s) printf("SEED_COST_%d %a\n", s, SearchPolicy::SEED_COST[s]);
    printf("LIST_COST %a\n", SearchPolicy::LIST_COST);
    printf("PRUNE_PASS_COST %a\n", SearchPolicy::PRUNE_PASS_COST);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "--constants")) return constants();
    SearchPolicy p;
    char line[512], kind[32], name[64];
    int lineno = 0;
    long long M = 0, N = 0, dp = 0;
    while (fgets(line, sizeof line, stdin)) {
        ++lineno;
        if (sscanf(line, "%31s", kind) != 1 || kind[0] == '#') continue;
        const char *args = strstr(line, kind) + strlen(kind);
        long long a[3];
        double d[4];
        bool ok = true;
        if (!strcmp(kind, "opt")) {
            ok = sscanf(args, "%63s %lld", name, &a[0]) == 2;
            if (!ok) {}
            else if (!strcmp(name, "algorithm")) p.algorithm = (int)a[0];
            else if (!strcmp(name, "sweep_planes")) p.sweep_planes = (int)a[0];
            else if (!strcmp(name, "seed_stride")) p.seed_stride = (int)a[0];
            else if (!strcmp(name, "refine")) p.set_refine((int)a[0]);
            else if (!strcmp(name, "max_mean_candidates")) p.max_mean_candidates = a[0];
            else ok = false;
        } else if (!strcmp(kind, "reset")) {
            p.reset();
        } else if (!strcmp(kind, "shape")) {
            ok = sscanf(args, "%lld %lld %lld", &M, &N, &dp) == 3 && M >= 1 && N >= 1 && dp >= 1;
        } else if (!strcmp(kind, "allowed")) {
            printf("a %d\n", (int)(p.filter_allowed() && SearchPolicy::shape_ok(M, N, dp)));
        } else if (!strcmp(kind, "plan")) {
            ok = sscanf(args, "%lld %lld %lld", &a[0], &a[1], &a[2]) == 3 && M >= 1;
            if (ok) {
                if (a[1]) p.begin_epoch();
                const SearchPolicy::Plan pl = p.plan(M, N, dp, a[0] != 0, a[1] != 0, a[2] != 0);
                printf("p %d %d %d %d %d %d %d %d %d %d %a %d\n", pl.planes, (int)pl.seed_full, (int)pl.probe, (int)pl.retry,
                       (int)pl.hint_bound, pl.seed_stride, pl.sweep_planes, (int)pl.refine, pl.refine_rows, pl.timing_form,
                       pl.guard_mean, (int)p.last_hinted);
            }
        } else if (!strcmp(kind, "guarded")) {
            p.on_guarded();
        } else if (!strcmp(kind, "refine_timed")) {
            ok = sscanf(args, "%lld %lf", &a[0], &d[0]) == 2 && (a[0] == 0 || a[0] == 1);
            if (ok) { (void)p.take_timing_form(); p.refine_timed((int)a[0], d[0]); }
        } else if (!strcmp(kind, "observe")) {
            ok = sscanf(args, "%lf %lf %lf %lld %lf", &d[0], &d[1], &d[2], &a[0], &d[3]) == 5 && M >= 1;
            if (ok) {
                (void)p.take_timing_form();
                p.observe(d[0], d[1], d[2], (N + 127) / 128, M, dp, a[0] != 0, d[3]);
                print_state(p);
            }
        } else if (!strcmp(kind, "exact_epoch")) {
            if (sscanf(args, "%lld", &a[0]) != 1) a[0] = 1;
            for (long long e = 0; e < a[0]; ++e) {
                p.begin_epoch();
                p.on_exact_epoch();
                (void)p.take_timing_form();
                p.observe_unfiltered();
            }
            print_state(p);
        } else if (!strcmp(kind, "k2")) {
            ok = sscanf(args, "%lld", &a[0]) == 1;
            if (ok) printf("k %d %d\n", (int)p.k2_prunes(M), p.k2_seed_stride(a[0] != 0));
        } else if (!strcmp(kind, "query")) {
            int stride = 0, planes = 1;
            p.query_args(M, &stride, &planes);
            printf("q %d %d\n", stride, planes);
        } else if (!strcmp(kind, "cost")) {
            ok = sscanf(args, "%lld %lld %lf", &a[0], &a[1], &d[0]) == 3 && a[0] >= 0 && a[0] <= 2 && a[1] >= 0 && a[1] <= 3;
            if (ok) printf("c %a\n", SearchPolicy::model_cost((int)a[0], (int)a[1], d[0], M, N, dp));
        } else {
            ok = false;
        }
        if (!ok) { fprintf(stderr, "policy_replay: line %d: cannot read '%s'\n", lineno, line); return 2; }
        fflush(stdout);
    }
    return 0;
}
