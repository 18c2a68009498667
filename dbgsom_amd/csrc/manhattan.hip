// metric="manhattan" on gfx950: the best-matching-unit search, the distance matrix and the k nearest prototypes under
//
//   dist(x, w) = sum_k |x_k - w_k|                                          (float64, no square root, no clamp)
//
// Direct form: per (row, prototype) the sequential chain
//   t = x_k - w_k;  acc = acc + |t|,   k ascending,
// so a row that equals a prototype is at distance 0.0 exactly, and the bits of a (row, prototype) pair depend on
// nothing but that row and that prototype -- not on the batch, the grid, the rows that share a workgroup or the slab.
// There is no multiply in the chain: nothing for the compiler to contract, and three correctly rounded operations
// per entry that NumPy restates bit for bit.  Winners: lexicographic minimum on (dist, index) as everywhere in this
// library; a pair whose distance is not below +inf (a NaN or an infinity in the row) is never a winner (Best::push).
//
// Kernels: direct_bmu_kernel and direct_dist_kernel (direct_rows.h, the layout in which the lanes own prototypes)
// with AbsTerm and PlainFinish.  What the vector unit issues per (row, prototype, feature) is two v_add_f64: the
// negation of w and the absolute value of t are source modifiers.  float32 rows are widened (exactly) into the
// workspace first: widening inside the loop would be a third vector instruction per entry and wavefront.
#include <math.h>

#include <algorithm>

#include "direct_rows.h"

namespace dbgsom {

// ---- float32 rows: their float64 copy (N x d, no padding) -----------------------------------------------
__global__ __launch_bounds__(256) void l1_prepare_kernel(const float *__restrict__ X, int64_t N, int d, int64_t ldx,
                                                         double *__restrict__ Xw) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);   // one wavefront per row
    if (i >= N) return;
    const float *__restrict__ x = X + i * ldx;
    for (int c = lane; c < d; c += 64) Xw[i * (int64_t)d + c] = widen(x[c]);
}

// A slab of the selection has few rows (64 MiB of it at M = 1024 are 8192 rows: 512 workgroups), so its launch also
// divides the prototype blocks over blockIdx.y.
constexpr int64_t L1_SLAB_FILL_BLOCKS = 2048;   // slab form: the grid the launcher aims at (8 workgroups x 256 CUs)

// -------------------------------------------------------------------------------------------------------
// workspace: [Wt: d x ldwt float64 | float32 rows only: N x d float64]
static size_t l1_wt_bytes(int64_t d, int64_t M) { return align_up((size_t)d * (size_t)csr_wt_ld(M) * 8); }

size_t bmu_manhattan_workspace_bytes(int x_dtype, int64_t N, int64_t d, int64_t M) {
    if (N < 0 || d < 1 || M < 1) return 0;
    return l1_wt_bytes(d, M) + (x_dtype == DBGSOM_F32 ? align_up((size_t)N * d * 8) : 0);
}

int launch_manhattan_weights(const double *W, int64_t M, int64_t d, int64_t ldw, void *ws, hipStream_t s) {
    return launch_transpose_weights(W, M, d, ldw, static_cast<double *>(ws), csr_wt_ld(M), s);
}

// the rows as float64: float64 rows as they are, float32 rows widened behind Wt in the workspace
static int l1_rows64(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, int64_t M, void *ws,
                     const double **X64, int64_t *ld64, hipStream_t s) {
    if (x_dtype == DBGSOM_F64) {
        *X64 = static_cast<const double *>(X); *ld64 = ldx;
        return DBGSOM_OK;
    }
    double *Xw = reinterpret_cast<double *>(static_cast<char *>(ws) + l1_wt_bytes(d, M));
    hipLaunchKernelGGL(l1_prepare_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, (const float *)X, N, (int)d, ldx, Xw);
    *X64 = Xw; *ld64 = d;
    return launch_status("l1_prepare_kernel");
}

template <int K, int R>
struct L1Search { static constexpr auto kernel = direct_bmu_kernel<AbsTerm, PlainFinish, K, R>; };

// the search of N rows against the transposed prototypes launch_manhattan_weights left in front of `ws`
int launch_bmu_manhattan_rows(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, int64_t M, int k,
                              int64_t *idx, double *dist, void *ws, size_t ws_bytes, hipStream_t s) {
    TRY_STATUS(masked_check_shape(x_dtype, N, d, ldx, M, k));
    if (N == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(X && idx && dist && ws, "null pointer");
    TRY_STATUS(workspace_check("dbgsom_bmu_manhattan", ws_bytes, bmu_manhattan_workspace_bytes(x_dtype, N, d, M)));
    const double *X64;
    int64_t ld64;
    TRY_STATUS(l1_rows64(X, x_dtype, N, d, ldx, M, ws, &X64, &ld64, s));
    launch_bmu_rows<L1Search>(N, k, s, X64, N, (int)d, ld64, static_cast<const double *>(ws), csr_wt_ld(M), (int)M, idx, dist,
                              PlainFinish{});
    return launch_status("l1_bmu_kernel");   // (the text as it always was; the kernel is direct_bmu_kernel)
}

static int distances_manhattan_check(int x_dtype, int64_t N, int64_t d, int64_t ldx, int64_t M, int64_t ldo) {
    TRY_STATUS(masked_check_shape(x_dtype, N, d, ldx, M, 1));
    DBGSOM_REQUIRE(M <= DBGSOM_MAX_PROTOTYPES, "need 1 <= M <= DBGSOM_MAX_PROTOTYPES");
    DBGSOM_REQUIRE(ldo >= M, "ldo must be >= M");
    return DBGSOM_OK;
}

template <bool SLAB>
static int launch_distances_manhattan_form(const char *fn, const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx,
                                           int64_t M, double *out, int64_t ldo, void *ws, size_t ws_bytes, hipStream_t s) {
    TRY_STATUS(distances_manhattan_check(x_dtype, N, d, ldx, M, ldo));
    if (N == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(X && out && ws, "null pointer");
    DBGSOM_REQUIRE(is_aligned(out, 8), "out_dev must be 8-byte aligned");
    TRY_STATUS(workspace_check(fn, ws_bytes, bmu_manhattan_workspace_bytes(x_dtype, N, d, M)));
    const double *X64;
    int64_t ld64;
    TRY_STATUS(l1_rows64(X, x_dtype, N, d, ldx, M, ws, &X64, &ld64, s));
    const int64_t rb = N < MASKED_FEW_ROWS ? (N + MRS - 1) / MRS : (N + MR - 1) / MR, pb = (M + MT - 1) / MT;
    // slab form: as many shares of the prototype blocks as bring the grid to L1_SLAB_FILL_BLOCKS workgroups
    const unsigned gy = SLAB ? (unsigned)std::max<int64_t>(1, std::min(pb, (L1_SLAB_FILL_BLOCKS + rb - 1) / rb)) : 1u;
    launch_direct_dist<AbsTerm, PlainFinish, SLAB, true>(X64, N, d, ld64, static_cast<const double *>(ws), M, out, ldo,
                                                         PlainFinish{}, gy, s);
    return launch_status("l1_dist_kernel");   // (the text as it always was; the kernel is direct_dist_kernel)
}

int launch_distances_manhattan_rows(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, int64_t M, double *out,
                                    int64_t ldo, void *ws, size_t ws_bytes, hipStream_t s) {
    return launch_distances_manhattan_form<false>("dbgsom_distances_manhattan", X, x_dtype, N, d, ldx, M, out, ldo, ws,
                                                  ws_bytes, s);
}

// ---- the k nearest prototypes: slabs of rows, the selection of kneighbors.hip without its square root --------
// workspace: [that of bmu_manhattan_workspace_bytes for one slab of rows, Wt in front | the slab]
size_t kneighbors_manhattan_workspace_bytes(int x_dtype, int64_t N, int64_t d, int64_t M, int64_t slab_rows) {
    if (N < 1 || M < 1 || d < 1) return 0;
    return align_up(bmu_manhattan_workspace_bytes(x_dtype, kneighbors_slab_rows(N, M, slab_rows), d, M)) +
           kneighbors_workspace_bytes(N, M, slab_rows);
}

int kneighbors_manhattan_check(int x_dtype, int64_t N, int64_t d, int64_t ldx, int64_t M, int k, int64_t slab_rows) {
    TRY_STATUS(masked_check_shape(x_dtype, N, d, ldx, M, 1));
    DBGSOM_REQUIRE(M <= DBGSOM_MAX_PROTOTYPES, "need 1 <= M <= DBGSOM_MAX_PROTOTYPES");
    DBGSOM_REQUIRE(k >= 1 && k <= M, "need 1 <= k <= M");
    DBGSOM_REQUIRE(k <= DBGSOM_MAX_NEIGHBORS, "k must be <= DBGSOM_MAX_NEIGHBORS");
    DBGSOM_REQUIRE(slab_rows >= 0, "slab_rows must be >= 0 (0 = the default)");
    return DBGSOM_OK;
}

// the rows against the transposed prototypes launch_manhattan_weights left in front of `ws`
int launch_kneighbors_manhattan_rows(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, int64_t M, int k,
                                     int64_t slab_rows, int64_t *idx, double *dist, void *ws, size_t ws_bytes,
                                     hipStream_t s) {
    TRY_STATUS(kneighbors_manhattan_check(x_dtype, N, d, ldx, M, k, slab_rows));
    if (N == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(X && idx && dist && ws, "null pointer");
    TRY_STATUS(workspace_check("dbgsom_kneighbors_manhattan", ws_bytes,
                               kneighbors_manhattan_workspace_bytes(x_dtype, N, d, M, slab_rows)));
    DBGSOM_REQUIRE(is_aligned(ws, 16), "workspace_dev must be 16-byte aligned");
    const size_t front = align_up(bmu_manhattan_workspace_bytes(x_dtype, kneighbors_slab_rows(N, M, slab_rows), d, M));
    double *slab = reinterpret_cast<double *>(static_cast<char *>(ws) + front);
    return kneighbors_slabs(X, x_dtype, N, ldx, M, k, slab_rows, slab, launch_topk_rows_plain, idx, dist, s,
                            [&](const void *rows, int64_t, int64_t n, double *out, int64_t ldr) {
                                return launch_distances_manhattan_form<true>("dbgsom_kneighbors_manhattan", rows, x_dtype, n,
                                                                             d, ldx, M, out, ldr, ws, front, s);
                            });
}

}  // namespace dbgsom

using namespace dbgsom;

extern "C" {

size_t dbgsom_bmu_manhattan_workspace_bytes(int x_dtype, int64_t N, int64_t d, int64_t M) {
    return bmu_manhattan_workspace_bytes(x_dtype, N, d, M);
}

int dbgsom_bmu_manhattan(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *W_dev, int64_t M,
                         int64_t ldw, int k, int64_t *idx_dev, double *dist_dev, void *workspace_dev,
                         size_t workspace_bytes, void *stream) {
    TRY_STATUS(masked_check_shape(x_dtype, N, d, ldx, M, k));
    DBGSOM_REQUIRE(ldw >= d, "ldw must be >= d");
    if (N == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(X_dev && W_dev && idx_dev && dist_dev && workspace_dev, "null pointer");
    TRY_STATUS(workspace_check("dbgsom_bmu_manhattan", workspace_bytes, bmu_manhattan_workspace_bytes(x_dtype, N, d, M)));
    DBGSOM_REQUIRE(is_aligned(workspace_dev, 16), "workspace_dev must be 16-byte aligned");
    TRY_STATUS(launch_manhattan_weights(W_dev, M, d, ldw, workspace_dev, (hipStream_t)stream));
    return launch_bmu_manhattan_rows(X_dev, x_dtype, N, d, ldx, M, k, idx_dev, dist_dev, workspace_dev, workspace_bytes,
                                     (hipStream_t)stream);
}

int dbgsom_distances_manhattan(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *W_dev,
                               int64_t M, int64_t ldw, double *out_dev, int64_t ldo, void *workspace_dev,
                               size_t workspace_bytes, void *stream) {
    TRY_STATUS(distances_manhattan_check(x_dtype, N, d, ldx, M, ldo));
    DBGSOM_REQUIRE(ldw >= d, "ldw must be >= d");
    if (N == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(X_dev && W_dev && out_dev && workspace_dev, "null pointer");
    DBGSOM_REQUIRE(is_aligned(out_dev, 8), "out_dev must be 8-byte aligned");
    TRY_STATUS(workspace_check("dbgsom_distances_manhattan", workspace_bytes,
                               bmu_manhattan_workspace_bytes(x_dtype, N, d, M)));
    DBGSOM_REQUIRE(is_aligned(workspace_dev, 16), "workspace_dev must be 16-byte aligned");
    TRY_STATUS(launch_manhattan_weights(W_dev, M, d, ldw, workspace_dev, (hipStream_t)stream));
    return launch_distances_manhattan_rows(X_dev, x_dtype, N, d, ldx, M, out_dev, ldo, workspace_dev, workspace_bytes,
                                           (hipStream_t)stream);
}

size_t dbgsom_kneighbors_manhattan_workspace_bytes(int x_dtype, int64_t N, int64_t d, int64_t M, int64_t slab_rows) {
    return kneighbors_manhattan_workspace_bytes(x_dtype, N, d, M, slab_rows);
}

int dbgsom_kneighbors_manhattan(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *W_dev,
                                int64_t M, int64_t ldw, int k, int64_t slab_rows, int64_t *idx_dev, double *dist_dev,
                                void *workspace_dev, size_t workspace_bytes, void *stream) {
    TRY_STATUS(kneighbors_manhattan_check(x_dtype, N, d, ldx, M, k, slab_rows));
    DBGSOM_REQUIRE(ldw >= d, "ldw must be >= d");
    if (N == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(X_dev && W_dev && idx_dev && dist_dev && workspace_dev, "null pointer");
    TRY_STATUS(workspace_check("dbgsom_kneighbors_manhattan", workspace_bytes,
                               kneighbors_manhattan_workspace_bytes(x_dtype, N, d, M, slab_rows)));
    DBGSOM_REQUIRE(is_aligned(workspace_dev, 16), "workspace_dev must be 16-byte aligned");
    TRY_STATUS(launch_manhattan_weights(W_dev, M, d, ldw, workspace_dev, (hipStream_t)stream));
    return launch_kneighbors_manhattan_rows(X_dev, x_dtype, N, d, ldx, M, k, slab_rows, idx_dev, dist_dev, workspace_dev,
                                            workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
