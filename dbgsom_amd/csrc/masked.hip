// Query rows with missing entries (NaN) on gfx950: best-matching-unit search over the observed entries of
// each row, and the fill of the holes from the winner.
//
//   dist(x, w) = sqrt((d / n_obs) * sum_{k observed} (x_k - w_k)^2)        (prototypes are complete)
//
// scikit-learn's nan_euclidean convention; the factor is constant per row, so the winners are those of the
// plain sum over the observed entries.  Direct form in float64: per (row, prototype) the sequential chain
//   t = x_k - w_k;  acc = fma(t, t, acc),   k ascending over the observed entries,
// so a row that equals a prototype on its observed entries is at distance 0.0 exactly, and the bits of a
// (row, prototype) pair depend on nothing but that row and that prototype -- not on the batch, the grid,
// the rows that share a workgroup or the position of the prototype among the others.  Winners: lexicographic
// minimum on (sum, index) as everywhere in this library, then the scale and the square root.
//
// The N x M matrix of these distances is the same chain with every (row, prototype) stored.
//
// Kernels: masked_bmu_kernel below and direct_dist_kernel, on the pieces of direct_rows.h (the layout in which the
// lanes own prototypes) with SquaredObservedTerm and ObservedFinish.  The rows' entries arrive by scalar loads, the
// NaN test is integer arithmetic on the scalar unit and a missing entry is a uniform skip.  What the vector unit
// issues per (row, prototype, observed entry) is one v_add_f64 and one v_fma_f64.  float32 rows are widened (exactly)
// into the workspace first: widening inside the loop would be a third vector instruction per entry and wavefront.
#include <math.h>

#include "direct_rows.h"

namespace dbgsom {

// ---- per row: the number of observed entries, and (float32 rows) the float64 copy -------------------------
template <typename T>
__global__ __launch_bounds__(256) void masked_prepare_kernel(const T *__restrict__ X, int64_t N, int d, int64_t ldx,
                                                              int32_t *__restrict__ nobs, double *__restrict__ Xw) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);   // one wavefront per row
    if (i >= N) return;
    const T *__restrict__ x = X + i * ldx;
    int n = 0;
    for (int c = lane; c < d; c += 64) {
        const T v = x[c];
        n += (v == v) ? 1 : 0;
        if (Xw) Xw[i * (int64_t)d + c] = widen(v);
    }
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    if (lane == 0) nobs[i] = n;
}

// ---- search: direct_bmu_kernel (direct_rows.h) with SquaredObservedTerm and ObservedFinish, n_obs among its
// arguments.  A kernel of its own: merged into that one (n_obs behind the other arguments, inside the finish) it
// measured 0.2 % slower on 2e5 x 784 rows at 50 % missing, against the same library in the same visit.
template <int K, int R>
__global__ __launch_bounds__(MT) void masked_bmu_kernel(const double *__restrict__ X, int64_t N, int d, int64_t ldx,
                                                        const int32_t *__restrict__ nobs,
                                                        const double *__restrict__ Wt, int64_t ldwt, int M,
                                                        int64_t *__restrict__ idx_out, double *__restrict__ dist_out) {
    const int tid = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * R;
    const int nrows = (int)min((int64_t)R, N - i0);
    const double *__restrict__ xb = X + i0 * ldx;
    uint32_t off[R];   // (rows behind the last one repeat it: computed, never written; R ldx < 2^32 is required)
#pragma unroll
    for (int r = 0; r < R; ++r) off[r] = (uint32_t)min(r, nrows - 1) * (uint32_t)ldx;
    Best<K> best[R];
#pragma unroll
    for (int r = 0; r < R; ++r) best[r].init();

    for (int jb = 0; jb < M; jb += MT) {
        const int j = jb + tid;            // (j < ldwt: the columns behind M hold zeros)
        const double *__restrict__ wcol = Wt + j;
        double acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0.0;
        int e = 0;
        for (; e + MU <= d; e += MU) dense_step<SquaredObservedTerm, R, MU>(xb, off, e, wcol, ldwt, acc);
        for (; e < d; ++e) dense_step<SquaredObservedTerm, R, 1>(xb, off, e, wcol, ldwt, acc);
        if (j < M) {
#pragma unroll
            for (int r = 0; r < R; ++r) best[r].push(acc[r], j);
        }
    }
    const ObservedFinish<false> fin{nobs};
    DBGSOM_STORE_WINNERS(K, R, best, i0, nrows, d, fin, idx_out, dist_out);
}
template <int K, int R>
struct MaskedSearch { static constexpr auto kernel = masked_bmu_kernel<K, R>; };

// ---- X[i][c] = (T) W[idx[i]][c] wherever X[i][c] is NaN ---------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void fill_missing_kernel(T *__restrict__ X, int64_t N, int d, int64_t ldx,
                                                            const double *__restrict__ W, int64_t M, int64_t ldw,
                                                            const int64_t *__restrict__ idx, int64_t idx_stride) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);   // one wavefront per row
    if (i >= N) return;
    const int64_t j = idx[i * idx_stride];
    if (j < 0 || j >= M) return;   // (no winner: the row stays as it is)
    T *x = X + i * ldx;
    const double *__restrict__ w = W + j * ldw;
    for (int c = lane; c < d; c += 64) {
        const T v = x[c];
        if (v != v) x[c] = (T)w[c];
    }
}

// -------------------------------------------------------------------------------------------------------
static bool masked_dtype_ok(int dt) { return dt == DBGSOM_F32 || dt == DBGSOM_F64; }

// workspace: [Wt: d x ldwt float64 | n_obs: N int32 | float32 rows only: N x d float64]
static size_t masked_wt_bytes(int64_t d, int64_t M) { return align_up((size_t)d * (size_t)csr_wt_ld(M) * 8); }
static size_t masked_nobs_bytes(int64_t N) { return align_up((size_t)N * 4); }

size_t bmu_masked_workspace_bytes(int x_dtype, int64_t N, int64_t d, int64_t M) {
    if (N < 0 || d < 1 || M < 1) return 0;
    return masked_wt_bytes(d, M) + masked_nobs_bytes(N) + (x_dtype == DBGSOM_F32 ? align_up((size_t)N * d * 8) : 0);
}

int masked_check_shape(int x_dtype, int64_t N, int64_t d, int64_t ldx, int64_t M, int k) {
    DBGSOM_REQUIRE(masked_dtype_ok(x_dtype), "x_dtype must be DBGSOM_F32 or DBGSOM_F64");
    DBGSOM_REQUIRE(k == 1 || k == 2, "k must be 1 or 2");
    DBGSOM_REQUIRE(N >= 0 && N < 0x7fffffff && d >= 1 && ldx >= d, "bad sample shape");
    DBGSOM_REQUIRE(ldx <= ((int64_t)1 << 27), "rows longer than 2^27 values");   // (MR ldx fits 32 bits)
    DBGSOM_REQUIRE(M >= k && M <= 0x7fffff00, "need k <= M < 2^31");
    return DBGSOM_OK;
}

int launch_masked_weights(const double *W, int64_t M, int64_t d, int64_t ldw, void *ws, hipStream_t s) {
    return launch_transpose_weights(W, M, d, ldw, static_cast<double *>(ws), csr_wt_ld(M), s);
}

// The halves of a search, on their own for rows that stay where they are (the resident rows of a fit on incomplete
// data): what depends on the rows alone -- n_obs and, for float32 rows, the float64 copy (N x d, no padding) -- is
// made once per load, and every search reads it.
int launch_masked_prepare(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, int32_t *nobs, double *Xw,
                          hipStream_t s) {
    TRY_STATUS(masked_check_shape(x_dtype, N, d, ldx, 1, 1));
    if (N == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(X && nobs && (x_dtype == DBGSOM_F64 || Xw), "null pointer");
    const dim3 pgrid((unsigned)((N + 3) / 4));
    if (x_dtype == DBGSOM_F32)
        hipLaunchKernelGGL(masked_prepare_kernel<float>, pgrid, dim3(256), 0, s, (const float *)X, N, (int)d, ldx, nobs, Xw);
    else
        hipLaunchKernelGGL(masked_prepare_kernel<double>, pgrid, dim3(256), 0, s, (const double *)X, N, (int)d, ldx, nobs,
                           (double *)nullptr);
    return launch_status("masked_prepare_kernel");
}

// X64: the rows as float64 (ld64 values apart), nobs: their observed entries; Wt: launch_masked_weights' output
int launch_bmu_masked_prepared(const double *X64, int64_t N, int64_t d, int64_t ld64, const int32_t *nobs,
                               const double *Wt, int64_t M, int k, int64_t *idx, double *dist, hipStream_t s) {
    TRY_STATUS(masked_check_shape(DBGSOM_F64, N, d, ld64, M, k));
    if (N == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(X64 && nobs && Wt && idx && dist, "null pointer");
    launch_bmu_rows<MaskedSearch>(N, k, s, X64, N, (int)d, ld64, nobs, Wt, csr_wt_ld(M), (int)M, idx, dist);
    return launch_status("masked_bmu_kernel");
}

// The workspace of N rows, Wt in front of it, and the prepared rows in it.
struct MaskedRows {
    const double *Wt;    // launch_masked_weights' output
    int32_t *nobs;
    const double *X64;   // float64 rows as they are, float32 rows widened behind n_obs
    int64_t ld64;
    int prepare(const char *fn, const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, int64_t M, void *ws,
                size_t ws_bytes, hipStream_t s) {
        TRY_STATUS(workspace_check(fn, ws_bytes, bmu_masked_workspace_bytes(x_dtype, N, d, M)));
        char *p = static_cast<char *>(ws);
        Wt = reinterpret_cast<const double *>(p);
        nobs = reinterpret_cast<int32_t *>(p + masked_wt_bytes(d, M));
        double *Xw = reinterpret_cast<double *>(p + masked_wt_bytes(d, M) + masked_nobs_bytes(N));
        const bool f32 = x_dtype == DBGSOM_F32;
        X64 = f32 ? Xw : static_cast<const double *>(X);
        ld64 = f32 ? d : ldx;
        return launch_masked_prepare(X, x_dtype, N, d, ldx, nobs, f32 ? Xw : nullptr, s);
    }
};

// the search of N rows against the transposed prototypes launch_masked_weights left in front of `ws`
int launch_bmu_masked_rows(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, int64_t M, int k,
                           int64_t *idx, double *dist, void *ws, size_t ws_bytes, hipStream_t s) {
    TRY_STATUS(masked_check_shape(x_dtype, N, d, ldx, M, k));
    if (N == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(X && idx && dist && ws, "null pointer");
    MaskedRows r;
    TRY_STATUS(r.prepare("dbgsom_bmu_masked", X, x_dtype, N, d, ldx, M, ws, ws_bytes, s));
    return launch_bmu_masked_prepared(r.X64, N, d, r.ld64, r.nobs, r.Wt, M, k, idx, dist, s);
}

// ---- the N x M matrix: the same chain, same d / n_obs scale, same square root, every pair stored -------
static int distances_masked_check(int x_dtype, int64_t N, int64_t d, int64_t ldx, int64_t M, int64_t ldo) {
    TRY_STATUS(masked_check_shape(x_dtype, N, d, ldx, M, 1));
    DBGSOM_REQUIRE(M <= DBGSOM_MAX_PROTOTYPES, "need 1 <= M <= DBGSOM_MAX_PROTOTYPES");
    DBGSOM_REQUIRE(ldo >= M, "ldo must be >= M");
    return DBGSOM_OK;
}

// SQ: the slab form of kneighbors.hip (the scaled sum without its square root, ordinary stores)
template <bool SQ>
static int launch_distances_masked_form(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, int64_t M,
                                        double *out, int64_t ldo, void *ws, size_t ws_bytes, hipStream_t s) {
    TRY_STATUS(distances_masked_check(x_dtype, N, d, ldx, M, ldo));
    if (N == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(X && out && ws, "null pointer");
    MaskedRows r;
    TRY_STATUS(r.prepare("dbgsom_distances_masked", X, x_dtype, N, d, ldx, M, ws, ws_bytes, s));
    launch_direct_dist<SquaredObservedTerm, ObservedFinish<SQ>, SQ, false>(r.X64, N, d, r.ld64, r.Wt, M, out, ldo,
                                                                          ObservedFinish<SQ>{r.nobs}, 1u, s);
    return launch_status("masked_dist_kernel");   // (the text as it always was; the kernel is direct_dist_kernel)
}

int launch_distances_masked_rows(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, int64_t M, double *out,
                                 int64_t ldo, void *ws, size_t ws_bytes, hipStream_t s) {
    return launch_distances_masked_form<false>(X, x_dtype, N, d, ldx, M, out, ldo, ws, ws_bytes, s);
}

int launch_distances_masked_rows_squared(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, int64_t M,
                                         double *out, int64_t ldo, void *ws, size_t ws_bytes, hipStream_t s) {
    return launch_distances_masked_form<true>(X, x_dtype, N, d, ldx, M, out, ldo, ws, ws_bytes, s);
}

size_t masked_weights_bytes(int64_t d, int64_t M) { return masked_wt_bytes(d, M); }

int launch_fill_missing(void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *W, int64_t M,
                        int64_t ldw, const int64_t *idx, int64_t idx_stride, hipStream_t s) {
    DBGSOM_REQUIRE(masked_dtype_ok(x_dtype), "x_dtype must be DBGSOM_F32 or DBGSOM_F64");
    DBGSOM_REQUIRE(N >= 0 && N < 0x7fffffff && d >= 1 && d <= 0x7fffffff && ldx >= d, "bad sample shape");
    DBGSOM_REQUIRE(M >= 1 && ldw >= d && idx_stride >= 1, "bad prototype shape or index stride");
    if (N == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(X && W && idx, "null pointer");
    const dim3 grid((unsigned)((N + 3) / 4));
    if (x_dtype == DBGSOM_F32)
        hipLaunchKernelGGL(fill_missing_kernel<float>, grid, dim3(256), 0, s, (float *)X, N, (int)d, ldx, W, M, ldw, idx, idx_stride);
    else
        hipLaunchKernelGGL(fill_missing_kernel<double>, grid, dim3(256), 0, s, (double *)X, N, (int)d, ldx, W, M, ldw, idx, idx_stride);
    return launch_status("fill_missing_kernel");
}

}  // namespace dbgsom

using namespace dbgsom;

extern "C" {

size_t dbgsom_bmu_masked_workspace_bytes(int x_dtype, int64_t N, int64_t d, int64_t M) {
    return bmu_masked_workspace_bytes(x_dtype, N, d, M);
}

int dbgsom_bmu_masked(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *W_dev, int64_t M,
                      int64_t ldw, int k, int64_t *idx_dev, double *dist_dev, void *workspace_dev, size_t workspace_bytes,
                      void *stream) {
    TRY_STATUS(masked_check_shape(x_dtype, N, d, ldx, M, k));
    DBGSOM_REQUIRE(ldw >= d, "ldw must be >= d");
    if (N == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(X_dev && W_dev && idx_dev && dist_dev && workspace_dev, "null pointer");
    TRY_STATUS(workspace_check("dbgsom_bmu_masked", workspace_bytes, bmu_masked_workspace_bytes(x_dtype, N, d, M)));
    DBGSOM_REQUIRE(is_aligned(workspace_dev, 16), "workspace_dev must be 16-byte aligned");
    TRY_STATUS(launch_masked_weights(W_dev, M, d, ldw, workspace_dev, (hipStream_t)stream));
    return launch_bmu_masked_rows(X_dev, x_dtype, N, d, ldx, M, k, idx_dev, dist_dev, workspace_dev, workspace_bytes,
                                  (hipStream_t)stream);
}

int dbgsom_distances_masked(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *W_dev,
                            int64_t M, int64_t ldw, double *out_dev, int64_t ldo, void *workspace_dev,
                            size_t workspace_bytes, void *stream) {
    TRY_STATUS(distances_masked_check(x_dtype, N, d, ldx, M, ldo));
    DBGSOM_REQUIRE(ldw >= d, "ldw must be >= d");
    if (N == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(X_dev && W_dev && out_dev && workspace_dev, "null pointer");
    TRY_STATUS(workspace_check("dbgsom_distances_masked", workspace_bytes, bmu_masked_workspace_bytes(x_dtype, N, d, M)));
    DBGSOM_REQUIRE(is_aligned(workspace_dev, 16), "workspace_dev must be 16-byte aligned");
    TRY_STATUS(launch_masked_weights(W_dev, M, d, ldw, workspace_dev, (hipStream_t)stream));
    return launch_distances_masked_rows(X_dev, x_dtype, N, d, ldx, M, out_dev, ldo, workspace_dev, workspace_bytes,
                                        (hipStream_t)stream);
}

int dbgsom_fill_missing(void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *W_dev, int64_t M,
                        int64_t ldw, const int64_t *idx_dev, int64_t idx_stride, void *stream) {
    return launch_fill_missing(X_dev, x_dtype, N, d, ldx, W_dev, M, ldw, idx_dev, idx_stride, (hipStream_t)stream);
}

}  // extern "C"
