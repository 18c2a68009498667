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
// Layout (that of bmu_csr_kernel): the lanes of a workgroup own prototypes and read Wt, the transposed
// float64 prototypes (d x ldwt, zeros behind column M), so one feature is one coalesced 512-byte read per
// wavefront, shared by the R rows the workgroup walks.  The rows' entries are the same for every lane: they
// arrive by scalar loads, the NaN test is integer arithmetic on the scalar unit and a missing entry is a
// uniform skip.  What the vector unit issues per (row, prototype, observed entry) is one v_add_f64 and one
// v_fma_f64.  float32 rows are widened (exactly) into the workspace first: widening inside the loop would be
// a third vector instruction per entry and wavefront.
#include <math.h>

#include "bmu_common.h"
#include "masked_common.h"

#define TRY_STATUS(expr) do { int _rc = (expr); if (_rc != DBGSOM_OK) return _rc; } while (0)

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

template <int K, int R>
__global__ __launch_bounds__(MT) void masked_bmu_kernel(const double *__restrict__ X, int64_t N, int d, int64_t ldx,
                                                        const int32_t *__restrict__ nobs,
                                                        const double *__restrict__ Wt, int64_t ldwt, int M,
                                                        int64_t *__restrict__ idx_out, double *__restrict__ dist_out) {
    __shared__ double mv[MT / 64][R][K];
    __shared__ int mj[MT / 64][R][K];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
        for (; e + MU <= d; e += MU) masked_step<R, MU>(xb, off, e, wcol, ldwt, acc);
        for (; e < d; ++e) masked_step<R, 1>(xb, off, e, wcol, ldwt, acc);
        if (j < M) {
#pragma unroll
            for (int r = 0; r < R; ++r) best[r].push(acc[r], j);
        }
    }
    // the lanes of a wavefront, then the wavefronts, hold different prototypes of the same rows
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            double ov[K];
            int oj[K];
#pragma unroll
            for (int t = 0; t < K; ++t) {
                ov[t] = __shfl_xor(best[r].v[t], m, 64);
                oj[t] = __shfl_xor(best[r].j[t], m, 64);
            }
            best[r].merge(ov, oj);
        }
        if (lane == 0) {
#pragma unroll
            for (int t = 0; t < K; ++t) { mv[wave][r][t] = best[r].v[t]; mj[wave][r][t] = best[r].j[t]; }
        }
    }
    __syncthreads();
    if (tid < nrows) {
        Best<K> b;
#pragma unroll
        for (int t = 0; t < K; ++t) { b.v[t] = mv[0][tid][t]; b.j[t] = mj[0][tid][t]; }
#pragma unroll
        for (int w = 1; w < MT / 64; ++w) {
            double ov[K];
            int oj[K];
#pragma unroll
            for (int t = 0; t < K; ++t) { ov[t] = mv[w][tid][t]; oj[t] = mj[w][tid][t]; }
            b.merge(ov, oj);
        }
        const int64_t i = i0 + tid;
        const double scale = (double)d / (double)nobs[i];   // (no observed entry: 0 * inf, the distance is NaN)
#pragma unroll
        for (int t = 0; t < K; ++t) {
            idx_out[i * K + t] = (b.j[t] == 0x7fffffff) ? (int64_t)-1 : (int64_t)b.j[t];
            dist_out[i * K + t] = sqrt(b.v[t] * scale);
        }
    }
}

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

// the search of N rows against the transposed prototypes launch_masked_weights left in front of `ws`
int launch_bmu_masked_rows(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, int64_t M, int k,
                           int64_t *idx, double *dist, void *ws, size_t ws_bytes, hipStream_t s) {
    TRY_STATUS(masked_check_shape(x_dtype, N, d, ldx, M, k));
    if (N == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(X && idx && dist && ws, "null pointer");
    if (ws_bytes < bmu_masked_workspace_bytes(x_dtype, N, d, M)) {
        set_error("dbgsom_bmu_masked: workspace of %zu bytes, %zu needed", ws_bytes,
                  bmu_masked_workspace_bytes(x_dtype, N, d, M));
        return DBGSOM_ENOMEM;
    }
    char *p = static_cast<char *>(ws);
    const double *Wt = reinterpret_cast<const double *>(p);
    int32_t *nobs = reinterpret_cast<int32_t *>(p + masked_wt_bytes(d, M));
    double *Xw = reinterpret_cast<double *>(p + masked_wt_bytes(d, M) + masked_nobs_bytes(N));
    const dim3 pgrid((unsigned)((N + 3) / 4));
    const double *X64;
    int64_t ld64;
    if (x_dtype == DBGSOM_F32) {
        hipLaunchKernelGGL(masked_prepare_kernel<float>, pgrid, dim3(256), 0, s, (const float *)X, N, (int)d, ldx, nobs, Xw);
        X64 = Xw; ld64 = d;
    } else {
        hipLaunchKernelGGL(masked_prepare_kernel<double>, pgrid, dim3(256), 0, s, (const double *)X, N, (int)d, ldx, nobs,
                           (double *)nullptr);
        X64 = (const double *)X; ld64 = ldx;
    }
    TRY_STATUS(launch_status("masked_prepare_kernel"));
    const int64_t ldwt = csr_wt_ld(M);
#define DBGSOM_BMU_MASKED(KK, RR)                                                                                \
    hipLaunchKernelGGL((masked_bmu_kernel<KK, RR>), dim3((unsigned)((N + RR - 1) / RR)), dim3(MT), 0, s, X64, N, \
                       (int)d, ld64, nobs, Wt, ldwt, (int)M, idx, dist)
    if (N < MASKED_FEW_ROWS) { if (k == 1) DBGSOM_BMU_MASKED(1, MRS); else DBGSOM_BMU_MASKED(2, MRS); }
    else { if (k == 1) DBGSOM_BMU_MASKED(1, MR); else DBGSOM_BMU_MASKED(2, MR); }
#undef DBGSOM_BMU_MASKED
    return launch_status("masked_bmu_kernel");
}

// The two halves of launch_bmu_masked_rows on their own, for rows that stay where they are (the resident rows of a
// fit on incomplete data): what depends on the rows alone -- n_obs and, for float32 rows, the float64 copy
// (N x d, no padding) -- is made once per load, and every search reads it.
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
    const int64_t ldwt = csr_wt_ld(M);
#define DBGSOM_BMU_MASKED(KK, RR)                                                                                \
    hipLaunchKernelGGL((masked_bmu_kernel<KK, RR>), dim3((unsigned)((N + RR - 1) / RR)), dim3(MT), 0, s, X64, N, \
                       (int)d, ld64, nobs, Wt, ldwt, (int)M, idx, dist)
    if (N < MASKED_FEW_ROWS) { if (k == 1) DBGSOM_BMU_MASKED(1, MRS); else DBGSOM_BMU_MASKED(2, MRS); }
    else { if (k == 1) DBGSOM_BMU_MASKED(1, MR); else DBGSOM_BMU_MASKED(2, MR); }
#undef DBGSOM_BMU_MASKED
    return launch_status("masked_bmu_kernel");
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
    if (workspace_bytes < bmu_masked_workspace_bytes(x_dtype, N, d, M)) {
        set_error("dbgsom_bmu_masked: workspace of %zu bytes, %zu needed", workspace_bytes,
                  bmu_masked_workspace_bytes(x_dtype, N, d, M));
        return DBGSOM_ENOMEM;
    }
    TRY_STATUS(launch_masked_weights(W_dev, M, d, ldw, workspace_dev, (hipStream_t)stream));
    return launch_bmu_masked_rows(X_dev, x_dtype, N, d, ldx, M, k, idx_dev, dist_dev, workspace_dev, workspace_bytes,
                                  (hipStream_t)stream);
}

int dbgsom_fill_missing(void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *W_dev, int64_t M,
                        int64_t ldw, const int64_t *idx_dev, int64_t idx_stride, void *stream) {
    return launch_fill_missing(X_dev, x_dtype, N, d, ldx, W_dev, M, ldw, idx_dev, idx_stride, (hipStream_t)stream);
}

}  // extern "C"
