// Weighted geodesics over the lattice of a map on gfx950 (MI355X), and the combined error of Kaski and Lagus (1996)
// that is read off them: e_i = d1_i + G[b1_i, b2_i], the distance of row i to its best matching unit plus the length of
// the shortest path along the map from that unit to the second-best one.
//
// Three kernels:
//   edge_lengths_kernel         len(a, b) = sqrt(s), s = 0 and then, k ascending, t = W[a, k] - W[b, k], p = t * t,
//                               s = s + p: the subtraction, the product and the sum rounded on their own (never a fused
//                               multiply-add), so len(a, b) == len(b, a) bit for bit.  A lane per edge: the fold is
//                               sequential by definition.
//   geodesic_kernel             one source per workgroup, its distance vector in LDS as float64 bit patterns.
//   combined_error_rows_kernel  a lane per row: e = d1 + G[b1 * ldg + b2].
//
// G[s, t] is the minimum over lattice paths s = v0, .., vn = t of the left fold ((0 + len(v0, v1)) + len(v1, v2)) + ...
// in float64; G[s, s] = 0, +inf without a path.  Rounded addition of a non-negative length is monotone in the running
// sum, so that minimum is the least fixed point of dist[v] = min(dist[v], dist[u] + len(u, v)) from dist[s] = 0 and
// every relaxation order ends in the same bits.  G[s, t] and G[t, s] fold from different ends and differ in their last
// bits for most pairs: row s is the fold from s, and nothing is symmetrised.
//
// The form: PUSH over the undirected edge list.  The lanes of a workgroup take the edges e = t, t + nt, ...; for an
// edge (a, b, len) a lane reads dist[a] and dist[b] (relaxed atomic loads: one ds_read_b64 each), forms both candidates
// and lowers the far end with a 64-bit unsigned atomic minimum in LDS -- non-negative doubles and +inf order as their
// bit patterns, and a minimum commutes, so the vector after a round does not depend on which lane came first.  A round
// ends in a barrier that also ORs "some lane lowered something"; a round that lowered nothing saw a constant vector, so
// every edge satisfied the fixed-point inequality against it and the loop ends.  A value read mid-round is some path's
// fold, hence never below the fixed point; at most M - 1 rounds are run (Bellman-Ford's bound; a lane that sees a value
// lowered earlier in the same round only gets there sooner).  No CSR is built, degree is not bounded (a star is one
// atomic word under 2099 lanes' minima), and M = 16000 takes 125 KiB of the 160 KiB of LDS, which no second buffer
// would fit beside.
//
// Every edge index is checked against [0, M) before LDS is touched (status bit -> DBGSOM_ERANGE), a length that is
// NaN or negative is skipped (status bit -> DBGSOM_EINVAL); +inf is legal and connects nothing, self-loops are
// ignored, repeated edges are harmless.  The workspace is the status word; what it holds on entry does not matter.
#include <math.h>

#include <algorithm>

#include "common.h"

namespace dbgsom {

namespace {

constexpr int GEO_NT_SMALL = 256;         // lanes of a workgroup whose vector fits 64 KiB (several workgroups share a CU)
constexpr int GEO_NT_LARGE = 1024;        // ... and of one that has a CU's LDS to itself
constexpr size_t GEO_LDS_SMALL = 65536;   // dynamic LDS above this needs the function attribute
constexpr int EDGE_NT = 256;
constexpr int ROWS_NT = 256;
constexpr uint32_t GEO_ST_RANGE = 1u;     // status bits: an index outside [0, M)
constexpr uint32_t GEO_ST_LENGTH = 2u;    // a length that is NaN or negative
constexpr size_t GEO_WS_BYTES = 256;
constexpr unsigned long long GEO_INF = 0x7ff0000000000000ull;

}  // namespace

// edges: E pairs (a, b).  W: M rows of d values, ldw >= d apart.  len: E values.
__global__ __launch_bounds__(EDGE_NT) void edge_lengths_kernel(const double *__restrict__ W, int M, int d, int64_t ldw,
                                                               const int32_t *__restrict__ edges, int64_t E,
                                                               double *__restrict__ len, uint32_t *status) {
#pragma clang fp contract(off)
    const int64_t e = (int64_t)blockIdx.x * EDGE_NT + threadIdx.x;
    if (e >= E) return;
    const int a = edges[2 * e], b = edges[2 * e + 1];
    if ((unsigned)a >= (unsigned)M || (unsigned)b >= (unsigned)M) {   // (reads nothing through it)
        atomicOr(status, GEO_ST_RANGE);
        len[e] = NAN;
        return;
    }
    const double *__restrict__ wa = W + (int64_t)a * ldw, *__restrict__ wb = W + (int64_t)b * ldw;
    double s = 0.0;
    for (int k = 0; k < d; ++k) {
        const double t = __dsub_rn(wa[k], wb[k]);
        const double p = __dmul_rn(t, t);
        s = __dadd_rn(s, p);
    }
    len[e] = sqrt(s);
}

// G: S rows of M values, ldg >= M apart; row r is the source sources[r] (sources == nullptr: r).  dist: M words of LDS.
__global__ __launch_bounds__(GEO_NT_LARGE) void geodesic_kernel(const int32_t *__restrict__ edges,
                                                                const double *__restrict__ len, int E, int M,
                                                                const int32_t *__restrict__ sources,
                                                                double *__restrict__ G, int64_t ldg, uint32_t *status) {
    extern __shared__ unsigned long long geo_dist[];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int src = sources ? sources[blockIdx.x] : (int)blockIdx.x;
    if ((unsigned)src >= (unsigned)M) {   // (uniform over the workgroup: nobody reaches a barrier)
        if (tid == 0) atomicOr(status, GEO_ST_RANGE);
        return;
    }
    for (int v = tid; v < M; v += nt) geo_dist[v] = v == src ? 0ull : GEO_INF;
    __syncthreads();
    uint32_t bad = 0;
    const int rounds = M > 2 ? M - 1 : 1;   // at most M - 1 rounds (one at least: it is also what checks the edges)
    for (int round = 0; round < rounds; ++round) {
        int lowered = 0;
        for (int e = tid; e < E; e += nt) {
            const int a = edges[2 * e], b = edges[2 * e + 1];
            const double l = len[e];
            if ((unsigned)a >= (unsigned)M || (unsigned)b >= (unsigned)M) { bad |= GEO_ST_RANGE; continue; }
            if (!(l >= 0.0)) { bad |= GEO_ST_LENGTH; continue; }
            if (a == b) continue;
            const unsigned long long ua = __hip_atomic_load(&geo_dist[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const unsigned long long ub = __hip_atomic_load(&geo_dist[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            // (the sums stay >= +0.0 or +inf: their bit patterns order as they do)
            const unsigned long long cb = (unsigned long long)__double_as_longlong(__dadd_rn(__longlong_as_double((long long)ua), l));
            const unsigned long long ca = (unsigned long long)__double_as_longlong(__dadd_rn(__longlong_as_double((long long)ub), l));
            if (cb < ub) lowered |= atomicMin(&geo_dist[b], cb) > cb;
            if (ca < ua) lowered |= atomicMin(&geo_dist[a], ca) > ca;
        }
        if (!__syncthreads_or(lowered)) break;   // (uniform) a round over a constant vector: the fixed point
    }
    if (bad) atomicOr(status, bad);
    double *__restrict__ row = G + (int64_t)blockIdx.x * ldg;
    for (int v = tid; v < M; v += nt) row[v] = __longlong_as_double((long long)geo_dist[v]);
}

// idx2: N pairs (b1, b2).  dist: N rows whose first value is d1, ldd apart.  e: N values.
__global__ __launch_bounds__(ROWS_NT) void combined_error_rows_kernel(const int64_t *__restrict__ idx2,
                                                                      const double *__restrict__ dist, int64_t ldd, int64_t N,
                                                                      const double *__restrict__ G, int64_t ldg, int M,
                                                                      double *__restrict__ e, uint32_t *status) {
    const int64_t i = (int64_t)blockIdx.x * ROWS_NT + threadIdx.x;
    if (i >= N) return;
    const int64_t b1 = idx2[2 * i], b2 = idx2[2 * i + 1];
    if (b1 == -1 || b2 == -1) { e[i] = NAN; return; }
    if ((uint64_t)b1 >= (uint64_t)M || (uint64_t)b2 >= (uint64_t)M) {   // (reads nothing through it)
        atomicOr(status, GEO_ST_RANGE);
        e[i] = NAN;
        return;
    }
    e[i] = __dadd_rn(dist[i * ldd], G[b1 * ldg + b2]);
}

// ---------------------------------------------------------------------------------------------
size_t geodesics_workspace_bytes(int64_t M, int64_t E) {
    if (M < 1 || M > DBGSOM_MAX_PROTOTYPES || E < 0) return 0;
    return GEO_WS_BYTES;
}

// the status word after the kernels of `what`: blocking
static int read_status(const char *what, uint32_t *status_dev, int64_t M, hipStream_t s) {
    uint32_t status = 0;
    DBGSOM_HIP_CHECK(hipMemcpyAsync(&status, status_dev, 4, hipMemcpyDeviceToHost, s));
    DBGSOM_HIP_CHECK(hipStreamSynchronize(s));
    if (status & GEO_ST_RANGE) {
        set_error("%s: an index outside [0, %lld)", what, (long long)M);
        return DBGSOM_ERANGE;
    }
    if (status & GEO_ST_LENGTH) {
        set_error("%s: an edge length that is NaN or negative", what);
        return DBGSOM_EINVAL;
    }
    return DBGSOM_OK;
}

static int check_ws(const char *what, int64_t M, int64_t E, const void *ws, size_t ws_bytes) {
    const size_t need = geodesics_workspace_bytes(M, E);
    if (!ws) { set_error("%s: null pointer", what); return DBGSOM_EINVAL; }
    if (ws_bytes < need) {
        set_error("%s: workspace of %zu bytes, %zu needed", what, ws_bytes, need);
        return DBGSOM_ENOMEM;
    }
    if (!is_aligned(ws, 256)) { set_error("%s: workspace must be 256-byte aligned", what); return DBGSOM_EINVAL; }
    return DBGSOM_OK;
}

int launch_edge_lengths(const double *W, int64_t M, int64_t d, int64_t ldw, const int32_t *edges, int64_t E, double *len,
                        uint32_t *status, hipStream_t s) {
    if (E == 0) return DBGSOM_OK;
    const int64_t nb = (E + EDGE_NT - 1) / EDGE_NT;
    hipLaunchKernelGGL(edge_lengths_kernel, dim3((unsigned)nb), dim3(EDGE_NT), 0, s, W, (int)M, (int)d, ldw, edges, E, len,
                       status);
    return launch_status("edge_lengths_kernel");
}

int launch_geodesic_rows(const int32_t *edges, const double *len, int64_t E, int64_t M, const int32_t *sources, int64_t S,
                         double *G, int64_t ldg, uint32_t *status, hipStream_t s) {
    if (S == 0) return DBGSOM_OK;
    const size_t lds = (size_t)M * 8;
    const int nt = lds > GEO_LDS_SMALL ? GEO_NT_LARGE : GEO_NT_SMALL;
    // (before every launch: the attribute belongs to the device that is current, not to the process)
    DBGSOM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&geodesic_kernel),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(geodesic_kernel, dim3((unsigned)S), dim3(nt), lds, s, edges, len, (int)E, (int)M, sources, G, ldg,
                       status);
    return launch_status("geodesic_kernel");
}

int launch_combined_error_rows(const int64_t *idx2, const double *dist, int64_t ldd, int64_t N, const double *G, int64_t ldg,
                               int64_t M, double *e, uint32_t *status, hipStream_t s) {
    if (N == 0) return DBGSOM_OK;
    const int64_t nb = (N + ROWS_NT - 1) / ROWS_NT;
    hipLaunchKernelGGL(combined_error_rows_kernel, dim3((unsigned)nb), dim3(ROWS_NT), 0, s, idx2, dist, ldd, N, G, ldg, (int)M,
                       e, status);
    return launch_status("combined_error_rows_kernel");
}

int geodesics_status(const char *what, uint32_t *status_dev, int64_t M, hipStream_t s) {
    return read_status(what, status_dev, M, s);
}

}  // namespace dbgsom

using namespace dbgsom;

extern "C" {

size_t dbgsom_geodesics_workspace_bytes(int64_t M, int64_t E) { return geodesics_workspace_bytes(M, E); }

int dbgsom_edge_lengths(const double *W_dev, int64_t M, int64_t d, int64_t ldw, const int32_t *edges_dev, int64_t E,
                        double *len_dev, void *stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    DBGSOM_REQUIRE(M >= 1 && M <= DBGSOM_MAX_PROTOTYPES, "need 1 <= M <= DBGSOM_MAX_PROTOTYPES");
    DBGSOM_REQUIRE(d >= 1 && d <= 0x7fffffff && ldw >= d, "bad prototype shape (need 1 <= d <= ldw)");
    DBGSOM_REQUIRE(E >= 0 && E <= 0x7fffffff, "need 0 <= E < 2^31");
    if (E == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(W_dev && edges_dev && len_dev, "null pointer");
    DBGSOM_REQUIRE(is_aligned(W_dev, 8) && is_aligned(len_dev, 8) && is_aligned(edges_dev, 4), "pointers must be aligned");
    // (the call has no workspace: its status word is an allocation of its own, and the call is blocking)
    uint32_t *status = nullptr;
    DBGSOM_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&status), GEO_WS_BYTES));
    int rc = DBGSOM_OK;
    if (hipMemsetAsync(status, 0, 4, stream) != hipSuccess) { set_error("dbgsom_edge_lengths: memset failed"); rc = DBGSOM_EHIP; }
    if (rc == DBGSOM_OK) rc = launch_edge_lengths(W_dev, M, d, ldw, edges_dev, E, len_dev, status, stream);
    if (rc == DBGSOM_OK) rc = read_status("dbgsom_edge_lengths", status, M, stream);
    (void)hipFree(status);
    return rc;
}

int dbgsom_geodesics(const int32_t *edges_dev, const double *len_dev, int64_t E, int64_t M, const int32_t *sources_dev,
                     int64_t S, double *G_dev, int64_t ldg, void *ws, size_t ws_bytes, void *stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    DBGSOM_REQUIRE(M >= 1 && M <= DBGSOM_MAX_PROTOTYPES, "need 1 <= M <= DBGSOM_MAX_PROTOTYPES");
    DBGSOM_REQUIRE(E >= 0 && E <= 0x7fffffff, "need 0 <= E < 2^31");
    DBGSOM_REQUIRE(S >= 0 && S <= 0x7fffffff, "need 0 <= S < 2^31");
    DBGSOM_REQUIRE(sources_dev || S == M, "without a source list S must be M");
    DBGSOM_REQUIRE(ldg >= M, "ldg must be >= M");
    DBGSOM_REQUIRE(G_dev && (E == 0 || (edges_dev && len_dev)), "null pointer");
    DBGSOM_REQUIRE(is_aligned(G_dev, 8) && is_aligned(len_dev, 8) && is_aligned(edges_dev, 4) && is_aligned(sources_dev, 4),
                   "pointers must be aligned");
    TRY_STATUS(check_ws("dbgsom_geodesics", M, E, ws, ws_bytes));
    if (S == 0) return DBGSOM_OK;
    uint32_t *status = static_cast<uint32_t *>(ws);
    DBGSOM_HIP_CHECK(hipMemsetAsync(status, 0, 4, stream));
    TRY_STATUS(launch_geodesic_rows(edges_dev, len_dev, E, M, sources_dev, S, G_dev, ldg, status, stream));
    return read_status("dbgsom_geodesics", status, M, stream);   // (blocking: the status word decides the return code)
}

int dbgsom_combined_error_rows(const int64_t *idx2_dev, const double *dist_dev, int64_t ldd, int64_t N, const double *G_dev,
                               int64_t ldg, int64_t M, double *e_dev, void *stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    DBGSOM_REQUIRE(M >= 1 && M <= DBGSOM_MAX_PROTOTYPES, "need 1 <= M <= DBGSOM_MAX_PROTOTYPES");
    DBGSOM_REQUIRE(N >= 0 && N <= (int64_t)0x7fffffff * ROWS_NT, "bad sample shape");
    DBGSOM_REQUIRE(ldd >= 1, "ldd must be >= 1");
    DBGSOM_REQUIRE(ldg >= M, "ldg must be >= M");
    if (N == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(idx2_dev && dist_dev && G_dev && e_dev, "null pointer");
    DBGSOM_REQUIRE(is_aligned(idx2_dev, 8) && is_aligned(dist_dev, 8) && is_aligned(G_dev, 8) && is_aligned(e_dev, 8),
                   "pointers must be 8-byte aligned");
    uint32_t *status = nullptr;
    DBGSOM_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&status), GEO_WS_BYTES));
    int rc = DBGSOM_OK;
    if (hipMemsetAsync(status, 0, 4, stream) != hipSuccess) { set_error("dbgsom_combined_error_rows: memset failed"); rc = DBGSOM_EHIP; }
    if (rc == DBGSOM_OK) rc = launch_combined_error_rows(idx2_dev, dist_dev, ldd, N, G_dev, ldg, M, e_dev, status, stream);
    if (rc == DBGSOM_OK) rc = read_status("dbgsom_combined_error_rows", status, M, stream);
    (void)hipFree(status);
    return rc;
}

}  // extern "C"
