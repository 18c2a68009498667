// The anchor rows and their chain (dbgsom_amd/csrc/anchor_chain.h) on the CPU: cases on stdin, two lines of output
// per case (tests/anchor_seeds.py run_chain_check, tests/test_anchor_seeds_cpu.py).
//
//   N A D                     a sample set of N rows with A anchors of D features, followed by
//   A x D numbers             the anchor rows, one row per line (hexadecimal floats: no bit is lost on the way)
//                          -> rows  r_0 .. r_{A-1}     anchor_rows(N, A)
//                             chain p_0 .. p_{A-1}     chain_anchors on the rows numbered 0 .. A - 1: the permutation
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "anchor_chain.h"

int main() {
    long long N, A, D;
    while (scanf("%lld %lld %lld", &N, &A, &D) == 3) {
        if (A < 1 || A > N || D < 1) { fprintf(stderr, "bad case %lld %lld %lld\n", N, A, D); return 2; }
        std::vector<double> a((size_t)A * D);
        char tok[64];
        for (size_t i = 0; i < a.size(); ++i) {
            if (scanf("%63s", tok) != 1) { fprintf(stderr, "short case\n"); return 2; }
            char *end = nullptr;
            a[i] = strtod(tok, &end);
            if (end == tok || *end) { fprintf(stderr, "bad number %s\n", tok); return 2; }
        }
        const std::vector<int64_t> rows = dbgsom::anchor_rows(N, A);
        printf("rows");
        for (int64_t r : rows) printf(" %lld", (long long)r);
        printf("\n");
        std::vector<int64_t> perm((size_t)A);
        for (int64_t k = 0; k < A; ++k) perm[(size_t)k] = k;
        dbgsom::chain_anchors(a, A, D, perm);
        printf("chain");
        for (int64_t p : perm) printf(" %lld", (long long)p);
        printf("\n");
    }
    return 0;
}
