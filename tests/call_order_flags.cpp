// The flags of ResidentSearchState (csrc/epoch_control.h) behind one named transition, from both starts: what the
// `after` column of tests/call_order.py is held against (tests/test_call_order_cpu.py).  Host-only.
//   stdin:  one transition per line
//   stdout: "<transition> <hint_valid idx_valid bound_valid from all-false> <the same from all-true>"
// The all-true start is the state behind a frozen epoch under Wb[0]: the bound refers to buffer 0, the resident one.
#include <stdio.h>
#include <string.h>

#include "epoch_control.h"

using dbgsom::ResidentSearchState;

static bool apply(ResidentSearchState &s, const char *t) {
    if (!strcmp(t, "dense_search_done")) s.dense_search_done(0, 130);
    else if (!strcmp(t, "foreign_search_begun")) s.foreign_search_begun();
    else if (!strcmp(t, "foreign_search_done")) s.foreign_search_done();
    else if (!strcmp(t, "caller_winners_taken")) s.caller_winners_taken();
    else if (!strcmp(t, "sums_made")) s.sums_made(130);
    else if (!strcmp(t, "epoch_failed")) s.epoch_failed();
    else if (!strcmp(t, "hint_seeded")) s.hint_seeded(130);
    else if (!strcmp(t, "weights_replaced_bound")) s.weights_replaced(0);    // the matrix the bound refers to
    else if (!strcmp(t, "weights_replaced_other")) s.weights_replaced(1);
    else if (!strcmp(t, "bucket_order_rewritten")) s.bucket_order_rewritten();
    else if (!strcmp(t, "reset")) s.reset();
    else return false;
    return true;
}

int main() {
    char line[128];
    while (fgets(line, sizeof line, stdin)) {
        line[strcspn(line, "\r\n")] = 0;
        if (!line[0]) continue;
        ResidentSearchState lo, hi;
        hi.dense_search_done(0, 130);
        hi.sums_made(130);
        if (!(hi.hint_valid && hi.last_idx_valid && hi.dist_bound_valid)) { fprintf(stderr, "the all-true start is not all true\n"); return 2; }
        if (!apply(lo, line) || !apply(hi, line)) { fprintf(stderr, "unknown transition '%s'\n", line); return 2; }
        printf("%s %d %d %d %d %d %d\n", line, lo.hint_valid, lo.last_idx_valid, lo.dist_bound_valid, hi.hint_valid,
               hi.last_idx_valid, hi.dist_bound_valid);
    }
    return 0;
}
