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
// Layout (that of masked_bmu_kernel, masked.hip): the lanes of a workgroup own prototypes and read Wt, the transposed
// float64 prototypes (d x ldwt, zeros behind column M), so one feature is one coalesced 512-byte read per wavefront,
// shared by the R rows the workgroup walks.  The rows' entries are the same for every lane: they arrive by scalar
// loads, the next row's in flight.  What the vector unit issues per (row, prototype, feature) is two v_add_f64: the
// negation of w and the absolute value of t are source modifiers.  float32 rows are widened (exactly) into the
// workspace first: widening inside the loop would be a third vector instruction per entry and wavefront.
#include <math.h>

#include <algorithm>

#include "bmu_common.h"
#include "masked_common.h"

#define TRY_STATUS(expr) do { int _rc = (expr); if (_rc != DBGSOM_OK) return _rc; } while (0)

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

// U features of R rows against this lane's prototype: acc[r] goes on along its chain, k ascending
// (uniform: the same entries for every lane; the next row's load is in flight while this row is worked on)
template <int R, int U>
__device__ __forceinline__ void l1_step(const double *__restrict__ xb, const uint32_t (&off)[R], int e,
                                        const double *__restrict__ wcol, int64_t ldwt, double (&acc)[R]) {
    double w[U];
#pragma unroll
    for (int u = 0; u < U; ++u) w[u] = wcol[(int64_t)(e + u) * ldwt];
    double x[U], xn[U];
#pragma unroll
    for (int u = 0; u < U; ++u) xn[u] = (xb + (off[0] + (uint32_t)e))[u];
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = xn[u];
        if (r + 1 < R) {
#pragma unroll
            for (int u = 0; u < U; ++u) xn[u] = (xb + (off[r + 1] + (uint32_t)e))[u];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) acc[r] = acc[r] + fabs(x[u] - w[u]);
    }
}

template <int K, int R>
__global__ __launch_bounds__(MT) void l1_bmu_kernel(const double *__restrict__ X, int64_t N, int d, int64_t ldx,
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
        for (; e + MU <= d; e += MU) l1_step<R, MU>(xb, off, e, wcol, ldwt, acc);
        for (; e < d; ++e) l1_step<R, 1>(xb, off, e, wcol, ldwt, acc);
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
#pragma unroll
        for (int t = 0; t < K; ++t) {
            idx_out[i * K + t] = (b.j[t] == 0x7fffffff) ? (int64_t)-1 : (int64_t)b.j[t];
            dist_out[i * K + t] = b.v[t];
        }
    }
}

// ---- the same loop, every (row, prototype) stored -------------------------------------------------------
// The lanes own prototypes, so the 256 distances of a row and prototype block are contiguous: one 8-byte store per
// lane is a coalesced 512-byte store per wavefront whatever the alignment of `out` and ldo.  The full matrix is never
// read again here (non-temporal stores); the slab of the selection is read back at once (ordinary stores).  A slab has
// few rows (64 MiB of it at M = 1024 are 8192 rows: 512 workgroups), so its launch also divides the prototype blocks
// over blockIdx.y; a pair's chain does not depend on the workgroup that runs it.
constexpr int64_t L1_SLAB_FILL_BLOCKS = 2048;   // slab form: the grid the launcher aims at (8 workgroups x 256 CUs)
template <int R, bool SLAB>
__global__ __launch_bounds__(MT) void l1_dist_kernel(const double *__restrict__ X, int64_t N, int d, int64_t ldx,
                                                     const double *__restrict__ Wt, int64_t ldwt, int M,
                                                     double *__restrict__ out, int64_t ldo) {
    const int tid = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * R;
    const int nrows = (int)min((int64_t)R, N - i0);
    const double *__restrict__ xb = X + i0 * ldx;
    uint32_t off[R];   // (rows behind the last one repeat it: computed, never written; R ldx < 2^32 is required)
#pragma unroll
    for (int r = 0; r < R; ++r) off[r] = (uint32_t)min(r, nrows - 1) * (uint32_t)ldx;
    for (int jb = (int)blockIdx.y * MT; jb < M; jb += (int)gridDim.y * MT) {
        const int j = jb + tid;            // (j < ldwt: the columns behind M hold zeros)
        const double *__restrict__ wcol = Wt + j;
        double acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0.0;
        int e = 0;
        for (; e + MU <= d; e += MU) l1_step<R, MU>(xb, off, e, wcol, ldwt, acc);
        for (; e < d; ++e) l1_step<R, 1>(xb, off, e, wcol, ldwt, acc);
        if (j < M) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (r < nrows) {
                    double *p = out + (i0 + r) * ldo + j;
                    if constexpr (SLAB) *p = acc[r];
                    else __builtin_nontemporal_store(acc[r], p);
                }
            }
        }
    }
}

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

static int l1_workspace_check(const char *fn, size_t have, size_t need) {
    if (have < need) {
        set_error("%s: workspace of %zu bytes, %zu needed", fn, have, need);
        return DBGSOM_ENOMEM;
    }
    return DBGSOM_OK;
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

// the search of N rows against the transposed prototypes launch_manhattan_weights left in front of `ws`
int launch_bmu_manhattan_rows(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, int64_t M, int k,
                              int64_t *idx, double *dist, void *ws, size_t ws_bytes, hipStream_t s) {
    TRY_STATUS(masked_check_shape(x_dtype, N, d, ldx, M, k));
    if (N == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(X && idx && dist && ws, "null pointer");
    TRY_STATUS(l1_workspace_check("dbgsom_bmu_manhattan", ws_bytes, bmu_manhattan_workspace_bytes(x_dtype, N, d, M)));
    const double *X64;
    int64_t ld64;
    TRY_STATUS(l1_rows64(X, x_dtype, N, d, ldx, M, ws, &X64, &ld64, s));
    const double *Wt = static_cast<const double *>(ws);
    const int64_t ldwt = csr_wt_ld(M);
#define DBGSOM_BMU_L1(KK, RR)                                                                                   \
    hipLaunchKernelGGL((l1_bmu_kernel<KK, RR>), dim3((unsigned)((N + RR - 1) / RR)), dim3(MT), 0, s, X64, N, (int)d, \
                       ld64, Wt, ldwt, (int)M, idx, dist)
    if (N < MASKED_FEW_ROWS) { if (k == 1) DBGSOM_BMU_L1(1, MRS); else DBGSOM_BMU_L1(2, MRS); }
    else { if (k == 1) DBGSOM_BMU_L1(1, MR); else DBGSOM_BMU_L1(2, MR); }
#undef DBGSOM_BMU_L1
    return launch_status("l1_bmu_kernel");
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
    TRY_STATUS(l1_workspace_check(fn, ws_bytes, bmu_manhattan_workspace_bytes(x_dtype, N, d, M)));
    const double *X64;
    int64_t ld64;
    TRY_STATUS(l1_rows64(X, x_dtype, N, d, ldx, M, ws, &X64, &ld64, s));
    const double *Wt = static_cast<const double *>(ws);
    const int64_t ldwt = csr_wt_ld(M);
    const int64_t rb = N < MASKED_FEW_ROWS ? (N + MRS - 1) / MRS : (N + MR - 1) / MR, pb = (M + MT - 1) / MT;
    // slab form: as many shares of the prototype blocks as bring the grid to L1_SLAB_FILL_BLOCKS workgroups
    const unsigned gy = SLAB ? (unsigned)std::max<int64_t>(1, std::min(pb, (L1_SLAB_FILL_BLOCKS + rb - 1) / rb)) : 1u;
    if (N < MASKED_FEW_ROWS)
        hipLaunchKernelGGL((l1_dist_kernel<MRS, SLAB>), dim3((unsigned)rb, gy), dim3(MT), 0, s, X64, N, (int)d, ld64, Wt, ldwt,
                           (int)M, out, ldo);
    else
        hipLaunchKernelGGL((l1_dist_kernel<MR, SLAB>), dim3((unsigned)rb, gy), dim3(MT), 0, s, X64, N, (int)d, ld64, Wt, ldwt,
                           (int)M, out, ldo);
    return launch_status("l1_dist_kernel");
}

int launch_distances_manhattan_rows(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, int64_t M, double *out,
                                    int64_t ldo, void *ws, size_t ws_bytes, hipStream_t s) {
    return launch_distances_manhattan_form<false>("dbgsom_distances_manhattan", X, x_dtype, N, d, ldx, M, out, ldo, ws,
                                                  ws_bytes, s);
}

// ---- the k nearest prototypes: slabs of rows, the selection of kneighbors.hip without its square root --------
// rows of the slab M rounded up to even apart, so that every row starts on 16 bytes (as the squared forms)
static int64_t l1_slab_ld(int64_t M) { return M + (M & 1); }

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
    TRY_STATUS(l1_workspace_check("dbgsom_kneighbors_manhattan", ws_bytes,
                                  kneighbors_manhattan_workspace_bytes(x_dtype, N, d, M, slab_rows)));
    DBGSOM_REQUIRE(is_aligned(ws, 16), "workspace_dev must be 16-byte aligned");
    const int64_t rows = kneighbors_slab_rows(N, M, slab_rows), ldr = l1_slab_ld(M);
    const size_t front = align_up(bmu_manhattan_workspace_bytes(x_dtype, rows, d, M));
    double *slab = reinterpret_cast<double *>(static_cast<char *>(ws) + front);
    const size_t es = dtype_size(x_dtype);
    for (int64_t r0 = 0; r0 < N; r0 += rows) {
        const int64_t n = std::min(rows, N - r0);
        TRY_STATUS(launch_distances_manhattan_form<true>("dbgsom_kneighbors_manhattan",
                                                         static_cast<const char *>(X) + (size_t)r0 * ldx * es, x_dtype, n, d,
                                                         ldx, M, slab, ldr, ws, front, s));
        TRY_STATUS(launch_topk_rows_plain(slab, n, M, ldr, k, idx + r0 * k, dist + r0 * k, s));
    }
    return DBGSOM_OK;
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
    TRY_STATUS(l1_workspace_check("dbgsom_bmu_manhattan", workspace_bytes, bmu_manhattan_workspace_bytes(x_dtype, N, d, M)));
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
    TRY_STATUS(l1_workspace_check("dbgsom_distances_manhattan", workspace_bytes,
                                  bmu_manhattan_workspace_bytes(x_dtype, N, d, M)));
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
    TRY_STATUS(l1_workspace_check("dbgsom_kneighbors_manhattan", workspace_bytes,
                                  kneighbors_manhattan_workspace_bytes(x_dtype, N, d, M, slab_rows)));
    DBGSOM_REQUIRE(is_aligned(workspace_dev, 16), "workspace_dev must be 16-byte aligned");
    TRY_STATUS(launch_manhattan_weights(W_dev, M, d, ldw, workspace_dev, (hipStream_t)stream));
    return launch_kneighbors_manhattan_rows(X_dev, x_dtype, N, d, ldx, M, k, slab_rows, idx_dev, dist_dev, workspace_dev,
                                            workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
