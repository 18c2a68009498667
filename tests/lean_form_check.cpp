// The lean form of the anchor-marked search on the CPU: what a call resolves to with DBGSOM_ANCHOR_LISTS_ONLY
// (dbgsom_amd/csrc/filter_form.h) and when the engine asks for it (dbgsom_amd/csrc/lean_gate.h).  One command per
// line on stdin, one line of output each:
//   form FLAGS PLANES K REFINE_ROWS M HAS_HINT HAS_ANCHORS HAS_RUNS
//        -> "error MESSAGE", or "ok lists_only anchor_mark w_planes gap_nb prune_retry refine seed_stride marking exact PASS..."
//   record M GENERATION PLAN HANDED LONG     (an anchor-seeded epoch came back)            -> "recorded"
//   forget                                   (an epoch that was not anchor-seeded)         -> "forgotten"
//   allows M GENERATION PLAN RETRY REFINE    (the next anchor-seeded epoch: lean?)          -> "0" / "1"
//   key SEED_STRIDE SWEEP_PLANES             -> LeanGate::plan_key
// The three gate commands work on ONE gate, in the order of the lines.  tests/test_lean_form_cpu.py holds the answers.
#include <stdio.h>
#include <string.h>

#include "filter_form.h"
#include "lean_gate.h"

int main() {
    static const char *const pass_name[] = {"anchor_mark", "prune_grid", "prune_handed", "reseed", "prune_reseeded"};
    static const char *const marking[] = {"prune", "sweep4", "sweep_1_4", "sweep_2_2", "sweep_3_1"};
    static const char *const exact[] = {"k2", "beside_refine", "split", "all"};
    dbgsom::LeanGate gate;
    char cmd[32];
    while (scanf("%31s", cmd) == 1) {
        if (!strcmp(cmd, "form")) {
            int flags, planes, k, refine_rows, has_hint, has_anchors, has_runs;
            long long M;
            if (scanf("%i %d %d %d %lld %d %d %d", &flags, &planes, &k, &refine_rows, &M, &has_hint, &has_anchors, &has_runs) != 8)
                return 2;
            dbgsom::FilterForm f;
            const char *err = f.resolve(flags, planes, k, refine_rows, 100000, 784, M, has_hint != 0, has_anchors != 0,
                                        has_runs != 0);
            if (err) {
                printf("error %s\n", err);
                continue;
            }
            dbgsom::FilterForm::Pass p[4];
            const int n = f.prune_passes(p);
            printf("ok %d %d %d %d %d %d %d %s %s", (int)f.lists_only, (int)f.anchor_mark, (int)f.w_planes, f.gap_nb,
                   (int)f.prune_retry, (int)f.refine, f.seed_stride, marking[f.marking], exact[f.exact]);
            for (int i = 0; i < n; ++i) printf(" %s", pass_name[p[i]]);
            printf("\n");
        } else if (!strcmp(cmd, "record")) {
            long long M, gen;
            int plan;
            double handed, long_lists;
            if (scanf("%lld %lld %i %lf %lf", &M, &gen, &plan, &handed, &long_lists) != 5) return 2;
            gate.record(M, gen, plan, handed, long_lists);
            printf("recorded\n");
        } else if (!strcmp(cmd, "forget")) {
            gate.forget();
            printf("forgotten\n");
        } else if (!strcmp(cmd, "allows")) {
            long long M, gen;
            int plan, retry, refine;
            if (scanf("%lld %lld %i %d %d", &M, &gen, &plan, &retry, &refine) != 5) return 2;
            printf("%d\n", (int)gate.allows(M, gen, plan, retry != 0, refine != 0));
        } else if (!strcmp(cmd, "key")) {
            int stride, planes;
            if (scanf("%i %d", &stride, &planes) != 2) return 2;
            printf("%d\n", dbgsom::LeanGate::plan_key(stride, planes));
        } else {
            return 2;
        }
    }
    return 0;
}
