// The passes of the pruning form of the filtered search (dbgsom_amd/csrc/filter_form.h: FilterForm::anchor_mark,
// prune_passes) on the CPU: one call per line on stdin,
//   FLAGS PLANES K REFINE_ROWS M HAS_HINT HAS_ANCHORS HAS_RUNS
// one line of output each: "error MESSAGE", or
//   ok anchor_mark PASS... | reports: PASS...
// with the passes by name, in launch order, and behind the bar those that report long lists to the policy.
// tests/test_anchor_mark_policy_cpu.py holds the expected answers.
#include <stdio.h>

#include "filter_form.h"

int main() {
    static const char *const name[] = {"anchor_mark", "prune_grid", "prune_handed", "reseed", "prune_reseeded"};
    int flags, planes, k, refine_rows, has_hint, has_anchors, has_runs;
    long long M;
    while (scanf("%i %d %d %d %lld %d %d %d", &flags, &planes, &k, &refine_rows, &M, &has_hint, &has_anchors, &has_runs) == 8) {
        dbgsom::FilterForm f;
        const char *err = f.resolve(flags, planes, k, refine_rows, 100000, 784, M, has_hint != 0, has_anchors != 0,
                                    has_runs != 0);
        if (err) {
            printf("error %s\n", err);
            continue;
        }
        dbgsom::FilterForm::Pass p[4];
        const int n = f.prune_passes(p);
        printf("ok %d", (int)f.anchor_mark);
        for (int i = 0; i < n; ++i) printf(" %s", name[p[i]]);
        printf(" | reports:");
        for (int i = 0; i < n; ++i)
            if (dbgsom::FilterForm::reports_long_lists(p[i])) printf(" %s", name[p[i]]);
        printf("\n");
    }
    return 0;
}
