// The k nearest prototypes of every row on gfx950 (MI355X), 1 <= k <= DBGSOM_MAX_NEIGHBORS: the all-pairs search for
// any k, without the N x M matrix ever leaving the chip's caches.
//
// Two kernels per slab of rows, on one stream:
//   1. the squared form of distances.hip: r_ij = max((|x_i|^2 + (-2 <x_i, w_j>)) + |w_j|^2, 0) (rows with missing
//      entries: d / n_obs * sum over the observed (x_k - w_k)^2) of slab_rows x M pairs into the workspace, ordinary
//      stores;
//   2. topk_rows_kernel<K>: one wavefront per row picks the k smallest (r, j) in lexicographic order and stores
//      (sqrt(r), j).
// The selection is on r, not on its square root: two distinct r can share a square root, and the prototype with the
// larger r must not overtake by its lower index.  A pair whose r is not below +inf (NaN, +inf) is never reported, as
// in Best<K>::push; slots left unfilled hold (inf, -1).
//
// Selection.  Lane l streams the entries l, l + 64, ... of its row (coalesced, four loads in flight) into a sorted
// list of K (r, j) pairs in registers.  The index ascends per lane, so the strict '<' of the insertion keeps the
// lowest index first among equal r.  The insertion is an unrolled compare-and-shift chain; the list is never indexed
// by a run-time value, so it never leaves the registers.  Then k rounds: a wave-wide lexicographic arg-min over the
// lanes' heads (DPP within a row of 16 lanes, v_permlane16_swap / v_permlane32_swap across rows: no LDS), the lane
// whose head won pops it, lane t keeps round t's result.  The k results of a row go out as one store per array.
#include <math.h>

#include <algorithm>

#include "bmu_common.h"
#include "wave_lex.h"

namespace dbgsom {

constexpr int TOPK_NT = 256;              // four wavefronts, four rows per workgroup
constexpr int64_t KNEIGHBORS_SLAB_BYTES = (int64_t)64 << 20;
constexpr int64_t KNEIGHBORS_WAVE_ROWS = 512 * 128;

// R: N rows of M squared values, ldr >= M apart.  idx / dist: N x k, contiguous.  ROOT: the distance stored is the
// square root of the value selected on; without it the value itself (manhattan.hip: its slab holds distances).
template <int K, bool ROOT = true>
__global__ __launch_bounds__(TOPK_NT) void topk_rows_kernel(const double *__restrict__ R, int64_t N, int M, int64_t ldr,
                                                            int k, int64_t *__restrict__ idx, double *__restrict__ dist) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (TOPK_NT / 64) + (threadIdx.x >> 6);
    if (row >= N) return;   // (wave-uniform: the wavefronts that stay are whole)
    const double *__restrict__ p = R + row * ldr;

    SortedList<K> list;
    list.init();
    for (int j0 = lane; j0 < M + lane; j0 += 256) {   // (the trip count is wave-uniform; M + 63 + 256 < 2^31)
        double r[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int jj = j0 + 64 * u;
            r[u] = (jj < M) ? p[jj] : (double)INFINITY;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) list.push(r[u], j0 + 64 * u);
    }

    double mine = INFINITY;
    int mine_j = TOPK_EMPTY;
    for (int t = 0; t < k; ++t) {
        double bv = list.v[0];
        int bj = list.j[0];
        wave_lex_min(bv, bj);
        list.pop(bj == list.j[0] && bj != TOPK_EMPTY);   // (an index lives in one lane only)
        if (lane == t) { mine = bv; mine_j = bj; }
    }
    if (lane < k) {
        idx[row * k + lane] = (mine_j == TOPK_EMPTY) ? (int64_t)-1 : (int64_t)mine_j;
        dist[row * k + lane] = ROOT ? sqrt(mine) : mine;
    }
}

// ---------------------------------------------------------------------------------------------
static int topk_check(int64_t N, int64_t M, int64_t ldr, int k) {
    DBGSOM_REQUIRE(N >= 0, "bad sample shape");
    DBGSOM_REQUIRE(M >= 1 && M <= DBGSOM_MAX_PROTOTYPES, "need 1 <= M <= DBGSOM_MAX_PROTOTYPES");
    DBGSOM_REQUIRE(k >= 1 && k <= M, "need 1 <= k <= M");
    DBGSOM_REQUIRE(k <= DBGSOM_MAX_NEIGHBORS, "k must be <= DBGSOM_MAX_NEIGHBORS");
    DBGSOM_REQUIRE(ldr >= M, "ldr must be >= M");
    return DBGSOM_OK;
}

template <bool ROOT>
static int launch_topk_form(const double *R, int64_t N, int64_t M, int64_t ldr, int k, int64_t *idx, double *dist,
                            hipStream_t s) {
    TRY_STATUS(topk_check(N, M, ldr, k));
    if (N == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(R && idx && dist, "null pointer");
    DBGSOM_REQUIRE(is_aligned(R, 8) && is_aligned(idx, 8) && is_aligned(dist, 8), "pointers must be 8-byte aligned");
    const int64_t nb = (N + TOPK_NT / 64 - 1) / (TOPK_NT / 64);
    DBGSOM_REQUIRE(nb <= 0x7fffffff, "too many samples for one launch");
    dim3 grid((unsigned)nb), block(TOPK_NT);
#define DBGSOM_TOPK(K) \
    hipLaunchKernelGGL((topk_rows_kernel<K, ROOT>), grid, block, 0, s, R, N, (int)M, ldr, k, idx, dist)
    if (k <= 1) DBGSOM_TOPK(1);
    else if (k <= 2) DBGSOM_TOPK(2);
    else if (k <= 4) DBGSOM_TOPK(4);
    else if (k <= 8) DBGSOM_TOPK(8);
    else if (k <= 16) DBGSOM_TOPK(16);
    else DBGSOM_TOPK(32);
#undef DBGSOM_TOPK
    return launch_status("topk_rows_kernel");
}

int launch_topk_rows(const double *R, int64_t N, int64_t M, int64_t ldr, int k, int64_t *idx, double *dist,
                     hipStream_t s) {
    return launch_topk_form<true>(R, N, M, ldr, k, idx, dist, s);
}

// the same selection on a matrix of distances: what is stored is the value selected on, no square root
int launch_topk_rows_plain(const double *R, int64_t N, int64_t M, int64_t ldr, int k, int64_t *idx, double *dist,
                           hipStream_t s) {
    return launch_topk_form<false>(R, N, M, ldr, k, idx, dist, s);
}

// The default: as many rows, in multiples of 128, as keep the slab at 64 MiB -- and where that is more than one full
// grid of the product kernel (KNEIGHBORS_WAVE_ROWS: two workgroups of 128 rows on each of 256 CUs), whole grids only:
// 655 workgroups run as long as 1024 do.
int64_t kneighbors_slab_rows(int64_t N, int64_t M, int64_t slab_rows) {
    if (slab_rows < 1) {
        slab_rows = std::max<int64_t>(128, KNEIGHBORS_SLAB_BYTES / (kneighbors_slab_ld(M) * 8) / 128 * 128);
        if (slab_rows > KNEIGHBORS_WAVE_ROWS) slab_rows = slab_rows / KNEIGHBORS_WAVE_ROWS * KNEIGHBORS_WAVE_ROWS;
    }
    return std::max<int64_t>(1, std::min(slab_rows, N));
}

size_t kneighbors_workspace_bytes(int64_t N, int64_t M, int64_t slab_rows) {
    if (N < 1 || M < 1) return 0;
    return align_up((size_t)kneighbors_slab_rows(N, M, slab_rows) * (size_t)kneighbors_slab_ld(M) * 8);
}

int launch_kneighbors(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx, const double *W,
                      int64_t M, const double *ww, int k, int64_t slab_rows, int64_t *idx, double *dist, void *ws,
                      size_t ws_bytes, hipStream_t s) {
    DBGSOM_REQUIRE(valid_dtype(x_dtype), "x_dtype must be DBGSOM_F32/F64/BF16");
    DBGSOM_REQUIRE(N >= 0 && d >= 1 && ldx >= d && d <= 0x7fffffff, "bad sample shape");
    TRY_STATUS(topk_check(N, M, M, k));
    DBGSOM_REQUIRE(slab_rows >= 0, "slab_rows must be >= 0 (0 = the default)");
    if (N == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(X && xx && W && ww && idx && dist && ws, "null pointer");
    TRY_STATUS(kneighbors_workspace_check("dbgsom_kneighbors", N, M, slab_rows, ws, ws_bytes, 0));
    return euclidean_slabs(X, x_dtype, N, d, ldx, xx, W, M, ww, slab_rows, static_cast<double *>(ws), s,
                           [&](int64_t r0, int64_t n, const double *slab, int64_t ldr) {
                               return launch_topk_rows(slab, n, M, ldr, k, idx + r0 * k, dist + r0 * k, s);
                           });
}

// metric="cosine": slabs of the cosine matrix (u, v: cosine.hip), then the selection that stores what it selected on
int launch_kneighbors_cosine(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *u, const double *W,
                             int64_t M, const double *v, int k, int64_t slab_rows, int64_t *idx, double *dist, void *ws,
                             size_t ws_bytes, hipStream_t s) {
    DBGSOM_REQUIRE(x_dtype == DBGSOM_F32 || x_dtype == DBGSOM_F64, "x_dtype must be DBGSOM_F32 or DBGSOM_F64");
    DBGSOM_REQUIRE(N >= 0 && d >= 1 && ldx >= d && d <= 0x7fffffff, "bad sample shape");
    TRY_STATUS(topk_check(N, M, M, k));
    DBGSOM_REQUIRE(slab_rows >= 0, "slab_rows must be >= 0 (0 = the default)");
    if (N == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(X && u && W && v && idx && dist && ws, "null pointer");
    TRY_STATUS(kneighbors_workspace_check("dbgsom_kneighbors_cosine", N, M, slab_rows, ws, ws_bytes, 0));
    double *slab = static_cast<double *>(ws);
    return kneighbors_slabs(X, x_dtype, N, ldx, M, k, slab_rows, slab, launch_topk_rows_plain, idx, dist, s,
                            [&](const void *rows, int64_t r0, int64_t n, double *out, int64_t ldr) {
                                return launch_distances_cosine_slab(rows, x_dtype, n, d, ldx, u + r0, W, M, v, out, ldr, s);
                            });
}

// workspace: [that of bmu_masked_workspace_bytes for one slab of rows, Wt in front | the slab]
size_t kneighbors_masked_workspace_bytes(int x_dtype, int64_t N, int64_t d, int64_t M, int64_t slab_rows) {
    if (N < 1 || M < 1 || d < 1) return 0;
    return align_up(bmu_masked_workspace_bytes(x_dtype, kneighbors_slab_rows(N, M, slab_rows), d, M)) +
           kneighbors_workspace_bytes(N, M, slab_rows);
}

static int kneighbors_masked_check(int x_dtype, int64_t N, int64_t d, int64_t ldx, int64_t M, int k, int64_t slab_rows) {
    TRY_STATUS(masked_check_shape(x_dtype, N, d, ldx, M, 1));
    TRY_STATUS(topk_check(N, M, M, k));
    DBGSOM_REQUIRE(slab_rows >= 0, "slab_rows must be >= 0 (0 = the default)");
    return DBGSOM_OK;
}

// the rows against the transposed prototypes launch_masked_weights left in front of `ws`
int launch_kneighbors_masked_rows(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, int64_t M, int k,
                                  int64_t slab_rows, int64_t *idx, double *dist, void *ws, size_t ws_bytes,
                                  hipStream_t s) {
    TRY_STATUS(kneighbors_masked_check(x_dtype, N, d, ldx, M, k, slab_rows));
    if (N == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(X && idx && dist && ws, "null pointer");
    const size_t front = align_up(bmu_masked_workspace_bytes(x_dtype, kneighbors_slab_rows(N, M, slab_rows), d, M));
    TRY_STATUS(kneighbors_workspace_check("dbgsom_kneighbors_masked", N, M, slab_rows, ws, ws_bytes, front));
    double *slab = reinterpret_cast<double *>(static_cast<char *>(ws) + front);
    return kneighbors_slabs(X, x_dtype, N, ldx, M, k, slab_rows, slab, launch_topk_rows, idx, dist, s,
                            [&](const void *rows, int64_t, int64_t n, double *out, int64_t ldr) {
                                return launch_distances_masked_rows_squared(rows, x_dtype, n, d, ldx, M, out, ldr, ws, front, s);
                            });
}

}  // namespace dbgsom

using namespace dbgsom;

extern "C" {

int dbgsom_topk_rows(const double *R_dev, int64_t N, int64_t M, int64_t ldr, int k, int64_t *idx_dev, double *dist_dev,
                     void *stream) {
    return launch_topk_rows(R_dev, N, M, ldr, k, idx_dev, dist_dev, (hipStream_t)stream);
}

size_t dbgsom_kneighbors_workspace_bytes(int64_t N, int64_t M, int64_t slab_rows) {
    return kneighbors_workspace_bytes(N, M, slab_rows);
}

size_t dbgsom_kneighbors_masked_workspace_bytes(int x_dtype, int64_t N, int64_t d, int64_t M, int64_t slab_rows) {
    return kneighbors_masked_workspace_bytes(x_dtype, N, d, M, slab_rows);
}

int dbgsom_kneighbors(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx_dev,
                      const double *W_dev, int64_t M, const double *ww_dev, int k, int64_t slab_rows, int64_t *idx_dev,
                      double *dist_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    return launch_kneighbors(X_dev, x_dtype, N, d, ldx, xx_dev, W_dev, M, ww_dev, k, slab_rows, idx_dev, dist_dev,
                             workspace_dev, workspace_bytes, (hipStream_t)stream);
}

int dbgsom_kneighbors_masked(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *W_dev,
                             int64_t M, int64_t ldw, int k, int64_t slab_rows, int64_t *idx_dev, double *dist_dev,
                             void *workspace_dev, size_t workspace_bytes, void *stream) {
    TRY_STATUS(kneighbors_masked_check(x_dtype, N, d, ldx, M, k, slab_rows));
    DBGSOM_REQUIRE(ldw >= d, "ldw must be >= d");
    if (N == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(X_dev && W_dev && idx_dev && dist_dev && workspace_dev, "null pointer");
    const size_t front = align_up(bmu_masked_workspace_bytes(x_dtype, kneighbors_slab_rows(N, M, slab_rows), d, M));
    TRY_STATUS(kneighbors_workspace_check("dbgsom_kneighbors_masked", N, M, slab_rows, workspace_dev, workspace_bytes, front));
    TRY_STATUS(launch_masked_weights(W_dev, M, d, ldw, workspace_dev, (hipStream_t)stream));
    return launch_kneighbors_masked_rows(X_dev, x_dtype, N, d, ldx, M, k, slab_rows, idx_dev, dist_dev, workspace_dev,
                                         workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
