// The nearest stored rows of a query, through the map, on gfx950 (MI355X): an inverted-file scan.  The rows X are filed
// under units (the bucket order of dbgsom_ctx_partition: order / seg_start), a query names n_probe units (its nearest,
// dbgsom_ctx_kneighbors_query), and scan_cells_kernel looks at the rows filed under those units only.
//
// rho(i, q), the direct-form squared distance in float64 with a fixed order (include/dbgsom_hip.h): lane l of a
// wavefront owns partial l and takes the features l, l + 64, ... ascending, difference, product and sum each rounded on
// its own; six xor rounds (32, 16, 8, 4, 2, 1) then leave the same rho in every lane (a + b == b + a bit for bit).
//
// One workgroup of 256 lanes per query.  The query is widened into LDS once.  The candidates of the probed units are
// numbered 0 .. T - 1 in probe-list order; batch b (positions 64 b .. 64 b + 63) belongs to wavefront b % 4.  Lane l of
// the wavefront looks up the row of position 64 b + l (a scan over at most 32 prefix sums in LDS); the wavefront then
// walks the batch SCAN_ROWS rows at a time (their loads are independent: SCAN_ROWS coalesced segments of 64 values in
// flight per feature step), and the lane numbered by the candidate's position keeps its rho.  After the batch every
// lane inserts its one (rho, i) into its SortedList<K> -- push_lex: rows arrive in no order of i.  At the end K rounds
// of wave_lex_min select the wavefront's k best, the four wavefronts' lists meet in LDS, wavefront 0 reads them two
// per lane and selects once more; lanes 0 .. k - 1 store (sqrt(rho), i).  rho that is not below +inf (NaN, overflow)
// never enters a list; slots left unfilled hold (inf, -1).
//
// Nothing read from the caller's tables is followed blindly: a probe entry outside [0, M) is an empty cell, segment
// bounds are clamped to [0, N], a row number outside [0, N) is skipped.
//
// There is no split of one query's candidates over several workgroups: a single query with long cells runs on one CU.
#include <math.h>

#include <algorithm>

#include "bmu_common.h"
#include "wave_lex.h"

namespace dbgsom {

constexpr int SCAN_NT = 256;      // four wavefronts per query
constexpr int SCAN_WAVES = SCAN_NT / 64;
constexpr int SCAN_ROWS = 8;      // candidate rows in flight per wavefront
constexpr int SCAN_MAX_PROBE = DBGSOM_MAX_NEIGHBORS;

template <typename TX, typename TQ, int K>
__global__ __launch_bounds__(SCAN_NT) void scan_cells_kernel(const TX *__restrict__ X, int64_t N, int d, int64_t ldx,
                                                            const int32_t *__restrict__ order,
                                                            const uint32_t *__restrict__ seg_start, int M,
                                                            const TQ *__restrict__ Q, int64_t ldq,
                                                            const int64_t *__restrict__ probe, int n_probe, int k,
                                                            int64_t *__restrict__ idx, double *__restrict__ dist) {
    extern __shared__ double qs[];                      // the query, d doubles
    __shared__ int64_t cell_begin[SCAN_MAX_PROBE];      // where a probed cell starts in `order`
    __shared__ int64_t cell_cum[SCAN_MAX_PROBE + 1];    // candidates in front of it
    __shared__ double top_v[SCAN_WAVES * K];
    __shared__ int top_j[SCAN_WAVES * K];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q = blockIdx.x;
    const TQ *__restrict__ qrow = Q + q * ldq;
    for (int c = tid; c < d; c += SCAN_NT) qs[c] = (double)qrow[c];
    if (tid == 0) {
        int64_t cum = 0;
        for (int t = 0; t < n_probe; ++t) {
            const int64_t u = probe[q * n_probe + t];
            int64_t b = 0, e = 0;
            if (u >= 0 && u < M) {
                b = (int64_t)seg_start[u];
                e = (int64_t)seg_start[u + 1];
                b = b < N ? b : N;
                e = e < N ? e : N;
                e = e > b ? e : b;
            }
            cell_begin[t] = b;
            cell_cum[t] = cum;
            cum += e - b;
        }
        cell_cum[n_probe] = cum;
    }
    __syncthreads();
    const int64_t T = cell_cum[n_probe];

    SortedList<K> list;
    list.init();
    for (int64_t base = (int64_t)wave * 64; base < T; base += (int64_t)SCAN_WAVES * 64) {
        const int cnt = (int)(T - base < 64 ? T - base : 64);   // (wave-uniform)
        int row = -1;
        if (lane < cnt) {
            const int64_t pos = base + lane;
            int t = 0;
            while (t + 1 < n_probe && cell_cum[t + 1] <= pos) ++t;
            const int r = order[cell_begin[t] + (pos - cell_cum[t])];
            row = (r >= 0 && (int64_t)r < N) ? r : -1;
        }
        double mine = INFINITY;
        for (int u0 = 0; u0 < cnt; u0 += SCAN_ROWS) {
            const TX *__restrict__ xr[SCAN_ROWS];
            double p[SCAN_ROWS];
#pragma unroll
            for (int j = 0; j < SCAN_ROWS; ++j) {
                // (past the end of the batch: the batch's last row once more, kept by no lane that has a row)
                const int src = u0 + j < cnt ? u0 + j : cnt - 1;
                const int r = __shfl(row, src);
                xr[j] = X + (int64_t)(r > 0 ? r : 0) * ldx;
                p[j] = 0.0;
            }
            for (int c0 = 0; c0 < d; c0 += 64) {
                const int c = c0 + lane;
                const bool in = c < d;
                // (past d the lane loads the row's last value instead, so that no load sits behind a branch and all
                //  SCAN_ROWS stay in flight, and contributes t = 0: p + 0 is p)
                const int cl = in ? c : d - 1;
                const double qc = qs[cl];
                TX x[SCAN_ROWS];
#pragma unroll
                for (int j = 0; j < SCAN_ROWS; ++j) x[j] = xr[j][cl];
#pragma unroll
                for (int j = 0; j < SCAN_ROWS; ++j) {
                    const double t = in ? __dsub_rn((double)x[j], qc) : 0.0;
                    p[j] = __dadd_rn(p[j], __dmul_rn(t, t));
                }
            }
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
                for (int j = 0; j < SCAN_ROWS; ++j) p[j] = __dadd_rn(p[j], __shfl_xor(p[j], s));
            }
#pragma unroll
            for (int j = 0; j < SCAN_ROWS; ++j)
                if (lane == u0 + j) mine = p[j];
        }
        if (row >= 0) list.push_lex(mine, row);
    }

    // the wavefront's k best, round t's in lane t
    double best = INFINITY;
    int best_j = TOPK_EMPTY;
    for (int t = 0; t < k; ++t) {
        double bv = list.v[0];
        int bj = list.j[0];
        wave_lex_min(bv, bj);
        list.pop(bj == list.j[0] && bj != TOPK_EMPTY);   // (a row is filed under one unit: it lives in one lane only)
        if (lane == t) { best = bv; best_j = bj; }
    }
    if (lane < K) {
        top_v[wave * K + lane] = best;
        top_j[wave * K + lane] = best_j;
    }
    __syncthreads();
    if (wave != 0) return;

    // the four lists, two entries per lane, selected once more
    SortedList<2> two;
    two.init();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int e = lane + 64 * h;
        if (e < SCAN_WAVES * K) two.push_lex(top_v[e], top_j[e]);   // (an unfilled slot holds inf: it does not enter)
    }
    best = INFINITY;
    best_j = TOPK_EMPTY;
    for (int t = 0; t < k; ++t) {
        double bv = two.v[0];
        int bj = two.j[0];
        wave_lex_min(bv, bj);
        two.pop(bj == two.j[0] && bj != TOPK_EMPTY);
        if (lane == t) { best = bv; best_j = bj; }
    }
    if (lane < k) {
        idx[q * k + lane] = (best_j == TOPK_EMPTY) ? (int64_t)-1 : (int64_t)best_j;
        dist[q * k + lane] = sqrt(best);
    }
}

// ---------------------------------------------------------------------------------------------
int scan_cells_check(const char *fn, int x_dtype, int64_t N, int64_t d, int64_t ldx, int64_t M, int q_dtype, int64_t Nq,
                     int64_t ldq, int n_probe, int k) {
#define SCAN_REQUIRE(cond, msg) \
    do { if (!(cond)) { set_error("%s: %s", fn, msg); return DBGSOM_EINVAL; } } while (0)
    SCAN_REQUIRE((x_dtype == DBGSOM_F32 || x_dtype == DBGSOM_F64) && (q_dtype == DBGSOM_F32 || q_dtype == DBGSOM_F64),
                 "x_dtype and q_dtype must be DBGSOM_F32 or DBGSOM_F64");
    SCAN_REQUIRE(N >= 0 && N < 0x7fffffff && Nq >= 0 && Nq < 0x7fffffff && d >= 1, "bad sample shape");
    SCAN_REQUIRE(d <= DBGSOM_MAX_SCAN_FEATURES,
                 "rows of more than DBGSOM_MAX_SCAN_FEATURES = 8192 features are not scanned (the widened query lives in "
                 "64 KiB of LDS)");
    SCAN_REQUIRE(ldx >= d && ldq >= d, "ldx and ldq must be >= d");
    SCAN_REQUIRE(M >= 1 && M <= DBGSOM_MAX_PROTOTYPES, "need 1 <= M <= DBGSOM_MAX_PROTOTYPES");
    SCAN_REQUIRE(n_probe >= 1 && n_probe <= M && n_probe <= DBGSOM_MAX_NEIGHBORS,
                 "need 1 <= n_probe <= min(M, DBGSOM_MAX_NEIGHBORS)");
    SCAN_REQUIRE(k >= 1 && k <= DBGSOM_MAX_NEIGHBORS, "need 1 <= k <= DBGSOM_MAX_NEIGHBORS");
#undef SCAN_REQUIRE
    return DBGSOM_OK;
}

// one instantiation: its dynamic LDS may pass the default limit (asked for once)
template <typename TX, typename TQ, int K>
static int launch_scan_instance(const void *X, int64_t N, int d, int64_t ldx, const int32_t *order,
                                const uint32_t *seg_start, int M, const void *Q, int64_t Nq, int64_t ldq,
                                const int64_t *probe, int n_probe, int k, int64_t *idx, double *dist, hipStream_t s) {
    static bool attr_set = false;
    if (!attr_set) {
        DBGSOM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&scan_cells_kernel<TX, TQ, K>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, DBGSOM_MAX_SCAN_FEATURES * 8));
        attr_set = true;
    }
    hipLaunchKernelGGL((scan_cells_kernel<TX, TQ, K>), dim3((unsigned)Nq), dim3(SCAN_NT), (size_t)d * 8, s,
                       static_cast<const TX *>(X), N, d, ldx, order, seg_start, M, static_cast<const TQ *>(Q), ldq, probe,
                       n_probe, k, idx, dist);
    return DBGSOM_OK;
}

template <typename TX, typename TQ, typename... Args>
static int launch_scan_k(int k, Args... a) {
    if (k <= 1) return launch_scan_instance<TX, TQ, 1>(a...);
    if (k <= 2) return launch_scan_instance<TX, TQ, 2>(a...);
    if (k <= 4) return launch_scan_instance<TX, TQ, 4>(a...);
    if (k <= 8) return launch_scan_instance<TX, TQ, 8>(a...);
    if (k <= 16) return launch_scan_instance<TX, TQ, 16>(a...);
    return launch_scan_instance<TX, TQ, 32>(a...);
}

int launch_scan_cells(const char *fn, const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const int32_t *order,
                      const uint32_t *seg_start, int64_t M, const void *Q, int q_dtype, int64_t Nq, int64_t ldq,
                      const int64_t *probe, int n_probe, int k, int64_t *idx, double *dist, hipStream_t s) {
    TRY_STATUS(scan_cells_check(fn, x_dtype, N, d, ldx, M, q_dtype, Nq, ldq, n_probe, k));
    if (Nq == 0) return DBGSOM_OK;
    if (!((X || N == 0) && (order || N == 0) && seg_start && Q && probe && idx && dist)) {
        set_error("%s: null pointer", fn);
        return DBGSOM_EINVAL;
    }
    if (!(is_aligned(X, dtype_size(x_dtype)) && is_aligned(Q, dtype_size(q_dtype)) && is_aligned(order, 4) &&
          is_aligned(seg_start, 4) && is_aligned(probe, 8) && is_aligned(idx, 8) && is_aligned(dist, 8))) {
        set_error("%s: pointers must be aligned to their item size", fn);
        return DBGSOM_EINVAL;
    }
    const bool x32 = x_dtype == DBGSOM_F32, q32 = q_dtype == DBGSOM_F32;
    int rc;
#define DBGSOM_SCAN(TX, TQ) \
    rc = launch_scan_k<TX, TQ>(k, X, N, (int)d, ldx, order, seg_start, (int)M, Q, Nq, ldq, probe, n_probe, k, idx, dist, s)
    if (x32 && q32) DBGSOM_SCAN(float, float);
    else if (x32) DBGSOM_SCAN(float, double);
    else if (q32) DBGSOM_SCAN(double, float);
    else DBGSOM_SCAN(double, double);
#undef DBGSOM_SCAN
    if (rc != DBGSOM_OK) return rc;
    return launch_status("scan_cells_kernel");
}

}  // namespace dbgsom
