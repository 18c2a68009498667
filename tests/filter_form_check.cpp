// Resolves calls of the filtered search (dbgsom_amd/csrc/filter_form.h) on the CPU: one call per line on stdin,
//   FLAGS PLANES K REFINE_ROWS N D M HAS_HINT
// (FLAGS: the seed stride with DBGSOM_SEED_FULL / DBGSOM_PRUNE / DBGSOM_PRUNE_PROBE / DBGSOM_PRUNE_RETRY OR-ed in),
// one line of output each: "error MESSAGE", or
//   ok seed_full prune prune_probe prune_retry k2 seed_stride Msub Msubpad nkt_full nkt_used sweep_planes marking
//      gap_nb refine rows0 exact
// with `marking` and `exact` by name.  tests/test_filter_form_cpu.py holds the expected answers.
#include <stdio.h>

#include "filter_form.h"

int main() {
    static const char *const marking[] = {"prune", "sweep4", "sweep_1_4", "sweep_2_2", "sweep_3_1"};
    static const char *const exact[] = {"k2", "beside_refine", "split", "all"};
    int flags, planes, k, refine_rows, has_hint;
    long long N, d, M;
    while (scanf("%i %d %d %d %lld %lld %lld %d", &flags, &planes, &k, &refine_rows, &N, &d, &M, &has_hint) == 8) {
        dbgsom::FilterForm f;
        const char *err = f.resolve(flags, planes, k, refine_rows, N, d, M, has_hint != 0);
        if (err) {
            printf("error %s\n", err);
            continue;
        }
        printf("ok %d %d %d %d %d %d %d %d %d %d %d %s %d %d %d %s\n", (int)f.seed_full, (int)f.prune, (int)f.prune_probe,
               (int)f.prune_retry, (int)f.k2, f.seed_stride, f.Msub, f.Msubpad, f.nkt_full, f.nkt_used, f.sweep_planes,
               marking[f.marking], f.gap_nb, (int)f.refine, f.rows0, exact[f.exact]);
    }
    return 0;
}
