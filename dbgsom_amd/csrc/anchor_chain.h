// Which rows of a sample set become its anchors (filter.hip 2e, engine.hip ensure_anchors) and in which order they
// are numbered.  Host-only and free of HIP: rows in, row numbers out, so that the choice can be checked on any CPU
// (tests/anchor_chain_check.cpp, tests/test_anchor_seeds_cpu.py).  Results of a search never depend on any of this;
// the length of its candidate lists does.
#pragma once

#include <stdint.h>

#include <vector>

namespace dbgsom {

// A anchors of N rows: rows floor(k N / A), k = 0 .. A - 1 (A <= N: strictly increasing, row 0 first)
inline std::vector<int64_t> anchor_rows(int64_t N, int64_t A) {
    std::vector<int64_t> rows((size_t)A);
    for (int64_t k = 0; k < A; ++k) rows[(size_t)k] = k * N / A;
    return rows;
}

// The anchors are numbered along a greedy nearest-neighbour chain (from row 0 to the nearest anchor not yet taken,
// ties to the lower row; on the host, A^2 distances once per load): a 128-sample workgroup that straddles buckets
// then holds the samples of anchors that lie close together, where the strided rows themselves come in no order.
// a: the A anchor rows (A x dp float64) in the order of `rows`; rows: their row numbers, reordered in place.
inline void chain_anchors(const std::vector<double> &a, int64_t A, int64_t dp, std::vector<int64_t> &rows) {
    std::vector<double> d2((size_t)A * A, 0.0);
    for (int64_t i = 0; i < A; ++i)
        for (int64_t j = i + 1; j < A; ++j) {
            const double *x = &a[(size_t)i * dp], *y = &a[(size_t)j * dp];
            double acc = 0.0;
            for (int64_t k = 0; k < dp; ++k) { const double t = x[k] - y[k]; acc += t * t; }
            d2[(size_t)i * A + j] = d2[(size_t)j * A + i] = acc;
        }
    std::vector<char> taken((size_t)A, 0);
    std::vector<int64_t> chain;
    int64_t cur = 0;
    for (int64_t n = 0; n < A; ++n) {
        taken[(size_t)cur] = 1;
        chain.push_back(rows[(size_t)cur]);
        int64_t best = -1;
        for (int64_t j = 0; j < A; ++j)   // (a distance that is not a number is never the nearer one)
            if (!taken[(size_t)j] && (best < 0 || d2[(size_t)cur * A + j] < d2[(size_t)cur * A + best])) best = j;
        cur = best;
    }
    rows = chain;
}

}  // namespace dbgsom
