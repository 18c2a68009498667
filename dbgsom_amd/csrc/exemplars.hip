// The k nearest rows of X to every prototype on gfx950 (MI355X), 1 <= k <= DBGSOM_MAX_NEIGHBORS: the all-pairs search
// read down its columns, without the N x M matrix ever leaving the chip's caches.
//
// Per slab of rows, on one stream:
//   1. the squared form of distances.hip: r_ij = max((|x_i|^2 + (-2 <x_i, w_j>)) + |w_j|^2, 0) of slab_rows x M pairs
//      into the workspace, ordinary stores (what launch_kneighbors runs);
//   2. with own_cell, topk_rows_kernel<1> on the slab: the unit of every row, the index of its smallest (r_ij, j);
//   3. the fold (launch_topk_cols): per column j the k smallest (r_ij, i) in lexicographic order among what the state
//      held and the slab's rows, i the global row number.
// The state, M x k pairs (r float64, i int64) ascending with (+inf, -1) in unfilled slots, is carried from slab to slab
// and from chunk to chunk; (r, i) is a total order, so every partition of the rows gives the same selection.  One small
// kernel stores (sqrt(r), i) at the end: the selection is on r, as in kneighbors.hip.  A pair whose r is not below +inf
// (NaN, +inf) never enters a list.
//
// The fold is two kernels, three on long slabs of a small map.  The slab is row-major, so a wavefront reads it coalesced only when its lanes own adjacent
// columns, and M <= 1024 gives 1 .. 16 groups of 64 columns: the rows are split into segments of
// cols_segment(K) = max(64, 8 K) rows, one wavefront per (group, segment).
//   topk_cols_partial_kernel<K>  lane l owns column 64 g + l and walks its segment in ascending order, eight loads in
//       flight, into a SortedList<K> in registers (rows ascend, so the strict '<' keeps the lowest row among equal r).
//       With owners the owner of a row is wave-uniform, and only the lane whose column it names loads at all.  The
//       lane's list goes to the scratch as K pairs (r, int32 row within the call), laid out [column][segment][K]: each
//       lane stores K contiguous values, and the merge reads a column's candidates contiguously.
//   topk_cols_merge_kernel<K>    one wavefront per column, the skeleton of topk_rows_kernel: the lanes stream the
//       column's segments x K candidates and its k state entries into sorted lists -- the push compares (r, i), since
//       positions no longer order the rows -- and k rounds of wave_lex_min write the state back.  A column of more
//       than 2048 candidates (a slab of many rows: M <= 512 or so) is merged in two stages, since M wavefronts alone
//       leave most of the chip idle: parts of 512 candidates, one wavefront each, into lists of K in a second scratch,
//       then the final stage over those.
// The segment grows with K so that the scratch stays at or below 1.5 bytes per entry of the slab (12 K / max(64, 8 K)),
// while K <= 8 keeps 64 rows: 2048 wavefronts on a slab of 8192 x 1024.  The four wavefronts of a workgroup are not
// merged in LDS, and a wavefront takes one row at a time also where M <= 32 leaves lanes idle: DESIGN.md 4m.
#include <math.h>

#include <algorithm>

#include "wave_lex.h"

namespace dbgsom {

constexpr int COLS_NT = 256;       // four wavefronts per workgroup
constexpr int COLS_LOADS = 8;      // loads in flight per lane (segments are multiples of it)

static int cols_instance(int k) { return k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : k <= 8 ? 8 : k <= 16 ? 16 : 32; }
static int64_t cols_segment(int K) { return std::max(64, 8 * K); }
static int64_t cols_segments(int64_t N, int K) { return (N + cols_segment(K) - 1) / cols_segment(K); }
// parts of a column's S x K candidates in the first of two merge stages (1: one stage): a wavefront of the merge takes
// up to COLS_MERGE_ONE candidates alone, and beyond that the parts are of COLS_MERGE_PART
constexpr int64_t COLS_MERGE_ONE = 2048, COLS_MERGE_PART = 512;
static int64_t cols_parts(int64_t Q) { return Q <= COLS_MERGE_ONE ? 1 : (Q + COLS_MERGE_PART - 1) / COLS_MERGE_PART; }

// R: N rows of M squared values, ldr >= M apart.  owner: null or N units.  sr / si: M x S x K, the lists of column c's
// S segments one behind the other.
template <int K>
__global__ __launch_bounds__(COLS_NT) void topk_cols_partial_kernel(const double *__restrict__ R, int N, int M, int64_t ldr,
                                                                    const int64_t *__restrict__ owner, int seg_rows, int G,
                                                                    int64_t S, double *__restrict__ sr, int *__restrict__ si) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = (int64_t)blockIdx.x * (COLS_NT / 64) + (threadIdx.x >> 6);
    if (wid >= (int64_t)G * S) return;   // (wave-uniform: the wavefronts that stay are whole)
    const int g = (int)(wid % G);
    const int64_t seg = wid / G;
    const int c = 64 * g + lane;
    const bool live = c < M;
    const int begin = (int)(seg * seg_rows), end = (int)std::min<int64_t>(N, (seg + 1) * seg_rows);

    SortedList<K> list;
    list.init();
    for (int i0 = begin; i0 < end; i0 += COLS_LOADS) {
        double r[COLS_LOADS];
#pragma unroll
        for (int u = 0; u < COLS_LOADS; ++u) {
            const int i = i0 + u;
            bool take = live && i < end;
            if (owner) take = take && owner[i < end ? i : begin] == (int64_t)c;
            r[u] = take ? R[(int64_t)i * ldr + c] : (double)INFINITY;
        }
#pragma unroll
        for (int u = 0; u < COLS_LOADS; ++u) list.push(r[u], i0 + u);
    }
    if (live) {
        const int64_t at = ((int64_t)c * S + seg) * K;
#pragma unroll
        for (int t = 0; t < K; ++t) { sr[at + t] = list.v[t]; si[at + t] = list.j[t]; }
    }
}

// Column c, part p of P: the candidates p QP .. min(Q, (p + 1) QP) - 1 of the Q at sr / si + c Q -> their k smallest
// (r, i).  FINAL (P = 1): the column's k state entries are candidates too, row0 makes the rows global, and the result
// is written back to the state.  Otherwise it goes to out_r / out_i, laid out [column][part][K] as the input is, rows
// still within the call: the input of the final stage.
template <int K, bool FINAL>
__global__ __launch_bounds__(COLS_NT) void topk_cols_merge_kernel(const double *__restrict__ sr, const int *__restrict__ si,
                                                                  int M, int64_t Q, int64_t QP, int P, int row0, int k,
                                                                  double *state_r, int64_t *state_i,
                                                                  double *__restrict__ out_r, int *__restrict__ out_i) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = (int64_t)blockIdx.x * (COLS_NT / 64) + (threadIdx.x >> 6);
    if (wid >= (int64_t)M * P) return;   // (wave-uniform)
    const int c = (int)(wid / P), part = (int)(wid % P);
    const double *__restrict__ pr = sr + (int64_t)c * Q;
    const int *__restrict__ pi = si + (int64_t)c * Q;
    const int64_t begin = part * QP, end = std::min<int64_t>(Q, begin + QP);

    SortedList<K> list;
    list.init();
    if (FINAL && lane < k) {   // (r = +inf, an unfilled slot, never enters)
        const double r = state_r[(int64_t)c * k + lane];
        const int64_t i = state_i[(int64_t)c * k + lane];
        list.push_lex(r, (int)i);
    }
    for (int64_t q0 = begin + lane; q0 < end + lane; q0 += 256) {   // (the trip count is wave-uniform)
        double r[4];
        int i[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t q = q0 + 64 * u;
            r[u] = (q < end) ? pr[q] : (double)INFINITY;
            i[u] = (q < end) ? pi[q] : 0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) list.push_lex(r[u], (FINAL ? row0 : 0) + (r[u] < (double)INFINITY ? i[u] : 0));
    }

    double mine = INFINITY;
    int mine_i = TOPK_EMPTY;
    for (int t = 0; t < k; ++t) {
        double bv = list.v[0];
        int bi = list.j[0];
        wave_lex_min(bv, bi);
        list.pop(bi == list.j[0] && bi != TOPK_EMPTY);   // (a row lives in one lane only)
        if (lane == t) { mine = bv; mine_i = bi; }
    }
    if (FINAL) {
        if (lane < k) {
            state_r[(int64_t)c * k + lane] = mine;
            state_i[(int64_t)c * k + lane] = (mine_i == TOPK_EMPTY) ? (int64_t)-1 : (int64_t)mine_i;
        }
    } else if (lane < K) {   // (lanes k .. K - 1 hold (+inf, empty): every slot of the part is written)
        out_r[((int64_t)c * P + part) * K + lane] = mine;
        out_i[((int64_t)c * P + part) * K + lane] = mine_i;
    }
}

__global__ __launch_bounds__(COLS_NT) void topk_cols_init_kernel(double *__restrict__ state_r, int64_t *__restrict__ state_i,
                                                                 int n) {
    const int t = blockIdx.x * COLS_NT + threadIdx.x;
    if (t < n) { state_r[t] = INFINITY; state_i[t] = -1; }
}

// the state as the result: (sqrt(r), i)
__global__ __launch_bounds__(COLS_NT) void exemplars_store_kernel(const double *__restrict__ state_r,
                                                                  const int64_t *__restrict__ state_i, int n,
                                                                  int64_t *__restrict__ idx, double *__restrict__ dist) {
    const int t = blockIdx.x * COLS_NT + threadIdx.x;
    if (t < n) { dist[t] = sqrt(state_r[t]); idx[t] = state_i[t]; }
}

// ---------------------------------------------------------------------------------------------
static int cols_check(int64_t M, int k) {
    DBGSOM_REQUIRE(M >= 1 && M <= DBGSOM_MAX_PROTOTYPES, "need 1 <= M <= DBGSOM_MAX_PROTOTYPES");
    DBGSOM_REQUIRE(k >= 1, "need k >= 1");
    DBGSOM_REQUIRE(k <= DBGSOM_MAX_NEIGHBORS, "k must be <= DBGSOM_MAX_NEIGHBORS");
    return DBGSOM_OK;
}

// scratch of one fold: [r: M x S x K float64 | row: M x S x K int32 | with P > 1 parts: r: M x P x K | row: M x P x K]
static size_t cols_pairs_bytes(int64_t M, int64_t lists, int K, size_t item) {
    return align_up((size_t)M * (size_t)lists * (size_t)K * item);
}

size_t topk_cols_workspace_bytes(int64_t N, int64_t M, int k) {
    if (N < 1 || M < 1 || k < 1 || k > DBGSOM_MAX_NEIGHBORS) return 0;
    const int K = cols_instance(k);
    const int64_t S = cols_segments(N, K), P = cols_parts(S * K);
    return cols_pairs_bytes(M, S, K, 8) + cols_pairs_bytes(M, S, K, 4) +
           (P > 1 ? cols_pairs_bytes(M, P, K, 8) + cols_pairs_bytes(M, P, K, 4) : 0);
}

int launch_topk_cols_init(double *state_r, int64_t *state_i, int64_t M, int k, hipStream_t s) {
    TRY_STATUS(cols_check(M, k));
    DBGSOM_REQUIRE(state_r && state_i, "null pointer");
    DBGSOM_REQUIRE(is_aligned(state_r, 8) && is_aligned(state_i, 8), "pointers must be 8-byte aligned");
    const int n = (int)(M * k);
    hipLaunchKernelGGL(topk_cols_init_kernel, dim3((unsigned)((n + COLS_NT - 1) / COLS_NT)), dim3(COLS_NT), 0, s, state_r,
                       state_i, n);
    return launch_status("topk_cols_init_kernel");
}

int launch_topk_cols(const double *R, int64_t N, int64_t M, int64_t ldr, const int64_t *owner, int64_t row0, int k,
                     double *state_r, int64_t *state_i, void *ws, size_t ws_bytes, hipStream_t s) {
    DBGSOM_REQUIRE(N >= 0, "bad sample shape");
    TRY_STATUS(cols_check(M, k));
    DBGSOM_REQUIRE(ldr >= M, "ldr must be >= M");
    DBGSOM_REQUIRE(row0 >= 0 && row0 <= 0x7fffffff && N <= 0x7fffffff - row0, "need 0 <= row0 and row0 + N <= 2^31 - 1");
    if (N == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(R && state_r && state_i && ws, "null pointer");
    DBGSOM_REQUIRE(is_aligned(R, 8) && is_aligned(owner, 8) && is_aligned(state_r, 8) && is_aligned(state_i, 8),
                   "pointers must be 8-byte aligned");
    TRY_STATUS(workspace_check("dbgsom_topk_cols", ws_bytes, topk_cols_workspace_bytes(N, M, k)));
    DBGSOM_REQUIRE(is_aligned(ws, 16), "workspace_dev must be 16-byte aligned");
    const int K = cols_instance(k);
    const int64_t S = cols_segments(N, K), G = (M + 63) / 64, Q = S * K, P = cols_parts(Q);
    const int64_t nb = (G * S + COLS_NT / 64 - 1) / (COLS_NT / 64), nb1 = (M * P + COLS_NT / 64 - 1) / (COLS_NT / 64);
    DBGSOM_REQUIRE(nb <= 0x7fffffff && nb1 <= 0x7fffffff, "too many samples for one launch");
    char *base = static_cast<char *>(ws);
    double *sr = reinterpret_cast<double *>(base);
    int *si = reinterpret_cast<int *>(base + cols_pairs_bytes(M, S, K, 8));
    double *pr = reinterpret_cast<double *>(base + cols_pairs_bytes(M, S, K, 8) + cols_pairs_bytes(M, S, K, 4));
    int *pi = reinterpret_cast<int *>(reinterpret_cast<char *>(pr) + cols_pairs_bytes(M, P, K, 8));
    dim3 block(COLS_NT), pgrid((unsigned)nb), grid1((unsigned)nb1), mgrid((unsigned)((M + COLS_NT / 64 - 1) / (COLS_NT / 64)));
#define DBGSOM_COLS(KK)                                                                                              \
    do {                                                                                                             \
        hipLaunchKernelGGL((topk_cols_partial_kernel<KK>), pgrid, block, 0, s, R, (int)N, (int)M, ldr, owner,        \
                           (int)cols_segment(KK), (int)G, S, sr, si);                                                \
        TRY_STATUS(launch_status("topk_cols_partial_kernel"));                                                       \
        if (P > 1) {                                                                                                 \
            hipLaunchKernelGGL((topk_cols_merge_kernel<KK, false>), grid1, block, 0, s, sr, si, (int)M, Q,           \
                               COLS_MERGE_PART, (int)P, 0, k, nullptr, nullptr, pr, pi);                             \
            TRY_STATUS(launch_status("topk_cols_merge_kernel"));                                                     \
            hipLaunchKernelGGL((topk_cols_merge_kernel<KK, true>), mgrid, block, 0, s, pr, pi, (int)M, P * KK,       \
                               P * KK, 1, (int)row0, k, state_r, state_i, nullptr, nullptr);                         \
        } else {                                                                                                     \
            hipLaunchKernelGGL((topk_cols_merge_kernel<KK, true>), mgrid, block, 0, s, sr, si, (int)M, Q, Q, 1,      \
                               (int)row0, k, state_r, state_i, nullptr, nullptr);                                    \
        }                                                                                                            \
    } while (0)
    switch (K) {
    case 1: DBGSOM_COLS(1); break;
    case 2: DBGSOM_COLS(2); break;
    case 4: DBGSOM_COLS(4); break;
    case 8: DBGSOM_COLS(8); break;
    case 16: DBGSOM_COLS(16); break;
    default: DBGSOM_COLS(32); break;
    }
#undef DBGSOM_COLS
    return launch_status("topk_cols_merge_kernel");
}

int launch_exemplars_store(const double *state_r, const int64_t *state_i, int64_t M, int k, int64_t *idx, double *dist,
                           hipStream_t s) {
    TRY_STATUS(cols_check(M, k));
    DBGSOM_REQUIRE(state_r && state_i && idx && dist, "null pointer");
    DBGSOM_REQUIRE(is_aligned(idx, 8) && is_aligned(dist, 8), "pointers must be 8-byte aligned");
    const int n = (int)(M * k);
    hipLaunchKernelGGL(exemplars_store_kernel, dim3((unsigned)((n + COLS_NT - 1) / COLS_NT)), dim3(COLS_NT), 0, s, state_r,
                       state_i, n, idx, dist);
    return launch_status("exemplars_store_kernel");
}

// workspace of the slab loop: [the slab | the units of one slab's rows | their distances | the fold's scratch]
static size_t exemplars_owner_bytes(int64_t N, int64_t M, int64_t slab_rows) {
    return align_up((size_t)kneighbors_slab_rows(N, M, slab_rows) * 8);
}

size_t exemplars_fold_workspace_bytes(int64_t N, int64_t M, int k, int64_t slab_rows) {
    if (N < 1 || M < 1 || k < 1 || k > DBGSOM_MAX_NEIGHBORS) return 0;
    return kneighbors_workspace_bytes(N, M, slab_rows) + 2 * exemplars_owner_bytes(N, M, slab_rows) +
           topk_cols_workspace_bytes(kneighbors_slab_rows(N, M, slab_rows), M, k);
}

// ... and behind it the state: [r: M x k float64 | i: M x k int64]
static size_t exemplars_state_bytes(int64_t M, int k) { return align_up((size_t)M * (size_t)k * 8); }

size_t exemplars_workspace_bytes(int64_t N, int64_t M, int k, int64_t slab_rows) {
    if (M < 1 || k < 1 || k > DBGSOM_MAX_NEIGHBORS) return 0;
    return exemplars_fold_workspace_bytes(N, M, k, slab_rows) + 2 * exemplars_state_bytes(M, k);
}

static int exemplars_check(int x_dtype, int64_t N, int64_t d, int64_t ldx, int64_t M, int k, int64_t slab_rows, int64_t row0) {
    DBGSOM_REQUIRE(valid_dtype(x_dtype), "x_dtype must be DBGSOM_F32/F64/BF16");
    DBGSOM_REQUIRE(N >= 0 && d >= 1 && ldx >= d && d <= 0x7fffffff, "bad sample shape");
    TRY_STATUS(cols_check(M, k));
    DBGSOM_REQUIRE(slab_rows >= 0, "slab_rows must be >= 0 (0 = the default)");
    DBGSOM_REQUIRE(row0 >= 0 && row0 <= 0x7fffffff && N <= 0x7fffffff - row0, "need 0 <= row0 and row0 + N <= 2^31 - 1");
    return DBGSOM_OK;
}

// the Euclidean slab loop with the fold behind the product: rows row0 .. row0 + N - 1 into the state
int launch_exemplars_fold(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx, const double *W,
                          int64_t M, const double *ww, int k, int own_cell, int64_t slab_rows, int64_t row0, double *state_r,
                          int64_t *state_i, void *ws, size_t ws_bytes, hipStream_t s) {
    TRY_STATUS(exemplars_check(x_dtype, N, d, ldx, M, k, slab_rows, row0));
    if (N == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(X && xx && W && ww && state_r && state_i && ws, "null pointer");
    const size_t slab_bytes = kneighbors_workspace_bytes(N, M, slab_rows), own_bytes = exemplars_owner_bytes(N, M, slab_rows);
    const size_t scratch_bytes = topk_cols_workspace_bytes(kneighbors_slab_rows(N, M, slab_rows), M, k);
    TRY_STATUS(kneighbors_workspace_check("dbgsom_exemplars", N, M, slab_rows, ws, ws_bytes, 2 * own_bytes + scratch_bytes));
    char *base = static_cast<char *>(ws);
    int64_t *own = reinterpret_cast<int64_t *>(base + slab_bytes);
    double *own_dist = reinterpret_cast<double *>(base + slab_bytes + own_bytes);
    void *scratch = base + slab_bytes + 2 * own_bytes;
    return euclidean_slabs(X, x_dtype, N, d, ldx, xx, W, M, ww, slab_rows, reinterpret_cast<double *>(base), s,
                           [&](int64_t r0, int64_t n, const double *slab, int64_t ldr) {
                               if (own_cell) TRY_STATUS(launch_topk_rows(slab, n, M, ldr, 1, own, own_dist, s));
                               return launch_topk_cols(slab, n, M, ldr, own_cell ? own : nullptr, row0 + r0, k, state_r,
                                                       state_i, scratch, scratch_bytes, s);
                           });
}

int launch_exemplars(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx, const double *W,
                     int64_t M, const double *ww, int k, int own_cell, int64_t slab_rows, int64_t *idx, double *dist,
                     void *ws, size_t ws_bytes, hipStream_t s) {
    TRY_STATUS(exemplars_check(x_dtype, N, d, ldx, M, k, slab_rows, 0));
    DBGSOM_REQUIRE(idx && dist && ws && (N == 0 || (X && xx && W && ww)), "null pointer");
    DBGSOM_REQUIRE(is_aligned(idx, 8) && is_aligned(dist, 8), "pointers must be 8-byte aligned");
    const size_t front = exemplars_fold_workspace_bytes(N, M, k, slab_rows), need = exemplars_workspace_bytes(N, M, k, slab_rows);
    TRY_STATUS(workspace_check("dbgsom_exemplars", ws_bytes, need));
    DBGSOM_REQUIRE(is_aligned(ws, 16), "workspace_dev must be 16-byte aligned");
    double *state_r = reinterpret_cast<double *>(static_cast<char *>(ws) + front);
    int64_t *state_i = reinterpret_cast<int64_t *>(static_cast<char *>(ws) + front + exemplars_state_bytes(M, k));
    TRY_STATUS(launch_topk_cols_init(state_r, state_i, M, k, s));
    TRY_STATUS(launch_exemplars_fold(X, x_dtype, N, d, ldx, xx, W, M, ww, k, own_cell, slab_rows, 0, state_r, state_i, ws,
                                     front, s));
    return launch_exemplars_store(state_r, state_i, M, k, idx, dist, s);
}

}  // namespace dbgsom

using namespace dbgsom;

extern "C" {

size_t dbgsom_topk_cols_workspace_bytes(int64_t N, int64_t M, int k) { return topk_cols_workspace_bytes(N, M, k); }

int dbgsom_topk_cols_init(double *state_r_dev, int64_t *state_i_dev, int64_t M, int k, void *stream) {
    return launch_topk_cols_init(state_r_dev, state_i_dev, M, k, (hipStream_t)stream);
}

int dbgsom_topk_cols(const double *R_dev, int64_t N, int64_t M, int64_t ldr, const int64_t *owner_dev, int64_t row0, int k,
                     double *state_r_dev, int64_t *state_i_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    return launch_topk_cols(R_dev, N, M, ldr, owner_dev, row0, k, state_r_dev, state_i_dev, workspace_dev, workspace_bytes,
                            (hipStream_t)stream);
}

size_t dbgsom_exemplars_workspace_bytes(int64_t N, int64_t M, int k, int64_t slab_rows) {
    return exemplars_workspace_bytes(N, M, k, slab_rows);
}

int dbgsom_exemplars(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx_dev,
                     const double *W_dev, int64_t M, const double *ww_dev, int k, int own_cell, int64_t slab_rows,
                     int64_t *idx_dev, double *dist_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    return launch_exemplars(X_dev, x_dtype, N, d, ldx, xx_dev, W_dev, M, ww_dev, k, own_cell, slab_rows, idx_dev, dist_dev,
                            workspace_dev, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
