// Shared helpers of the gfx950 batch-SOM library (internal; the public ABI is include/dbgsom_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/dbgsom_hip.h"

namespace dbgsom {

void set_error(const char *fmt, ...);

#define DBGSOM_HIP_CHECK(expr)                                                           \
    do {                                                                                 \
        hipError_t _e = (expr);                                                          \
        if (_e != hipSuccess) {                                                          \
            ::dbgsom::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),   \
                                __FILE__, __LINE__);                                     \
            return DBGSOM_EHIP;                                                          \
        }                                                                                \
    } while (0)

#define DBGSOM_REQUIRE(cond, msg)                                   \
    do {                                                            \
        if (!(cond)) {                                              \
            ::dbgsom::set_error("%s: %s", __func__, msg);           \
            return DBGSOM_EINVAL;                                   \
        }                                                           \
    } while (0)

#define TRY_STATUS(expr) do { int _rc = (expr); if (_rc != DBGSOM_OK) return _rc; } while (0)

// `fn`: the public call whose workspace it is
inline int workspace_check(const char *fn, size_t have, size_t need) {
    if (have < need) {
        set_error("%s: workspace of %zu bytes, %zu needed", fn, have, need);
        return DBGSOM_ENOMEM;
    }
    return DBGSOM_OK;
}

inline int launch_status(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("launch of %s failed: %s", what, hipGetErrorString(e));
        return DBGSOM_EHIP;
    }
    return DBGSOM_OK;
}

// bfloat16 storage element: the upper 16 bits of a float32; widening is exact
struct bf16_t {
    uint16_t bits;
    __host__ __device__ bf16_t() = default;
    __host__ __device__ explicit bf16_t(int) : bits(0) {}
    __device__ __forceinline__ operator float() const { return __uint_as_float(((uint32_t)bits) << 16); }
};

// exact widening of a stored sample element to float64
__device__ __forceinline__ double widen(double v) { return v; }
__device__ __forceinline__ double widen(float v) { return (double)v; }
__device__ __forceinline__ double widen(bf16_t v) { return (double)(float)v; }

// "The last workgroup to finish does the follow-up step": folds a tiny dependent kernel (a scan
// over M entries, a final reduction) into the launch that produces its input -- a 4-5 us launch
// less per use.  Every workgroup calls this after its last global store; it returns true (in all
// threads) in exactly one workgroup, the one whose ticket is the last, and by then every other
// workgroup's stores are visible to it: plain stores -> every wave's vmcnt(0) -> barrier ->
// agent-scope release -> ticket (relaxed agent atomic); the last arriver: agent-scope acquire
// (invalidates this CU's L1) -> vmcnt(0) -> barrier -> plain loads (MI355X_MICROARCH.md,
// "Workgroup dispatch, XCD placement & inter-workgroup visibility").  The ticket counter must be 0
// before the launch; the last workgroup leaves it at 0 again.
__device__ __forceinline__ bool last_workgroup_done(uint32_t *ticket, uint32_t n_workgroups) {
    __shared__ int is_last_;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0 && threadIdx.z == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = (t == n_workgroups - 1u);
        if (last) {
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        is_last_ = last;
    }
    __syncthreads();
    return is_last_ != 0;
}

// A value loaded ahead of a guarded use counts as used where this stands: the compiler cannot move its load behind the
// guard (where it would be waited for on its own); the wait for the value moves up to here instead.
__device__ __forceinline__ void keep_load(const double &v) { asm volatile("" ::"v"(v)); }
__device__ __forceinline__ void keep_load(const float &v) { asm volatile("" ::"v"(v)); }

// change_total = sum_i rowchg[i] by ONE workgroup of 256 threads, in the fixed order of a 1024-leaf strided binary
// tree: leaf l adds rowchg[l], rowchg[l + 1024], ... in that order, thread t holds the leaves t + 256 u and joins
// them as (p0 + p2) + (p1 + p3) (tree levels 512 and 256), then the levels 128 .. 1 in LDS -- bitwise reproducible.
// The four leaves' loads of a trip go out together.  The sum is returned in thread 0.
__device__ __forceinline__ double change_total_tree(const double *__restrict__ rowchg, int M) {
    __shared__ double tot_[256];
    const int t = threadIdx.x;
    double p[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j0 = 0; j0 < M; j0 += 1024) {
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = rowchg[min(j0 + 256 * u + t, M - 1)];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            keep_load(v[u]);
            if (j0 + 256 * u + t < M) p[u] += v[u];
        }
    }
    tot_[t] = (p[0] + p[2]) + (p[1] + p[3]);
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) tot_[t] += tot_[t + w];
        __syncthreads();
    }
    return tot_[0];
}

inline bool valid_dtype(int dt) { return dt == DBGSOM_F32 || dt == DBGSOM_F64 || dt == DBGSOM_BF16; }
inline size_t dtype_size(int dt) { return dt == DBGSOM_F64 ? 8 : (dt == DBGSOM_F32 ? 4 : 2); }

inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }
inline bool is_aligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

// internal launchers (one per .hip file)
// per-stage timing of the topographic function (topofn.hip): the context call adds its search stage
bool topofn_timing_enabled();
void topofn_add_search_ms(double ms);
int launch_row_sqnorms(const void *A, int dtype, int64_t rows, int64_t d, int64_t ld, double *out,
                       hipStream_t s);
int launch_bmu(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx,
               const double *W, int64_t M, const double *ww, int k, int round_f32, int64_t *idx,
               double *dist, hipStream_t s);
int launch_exp_similarity(const double *dist, int64_t N, double gamma, double *kw, hipStream_t s);
size_t accumulate_workspace_bytes(int64_t N, int64_t d, int64_t M);
int launch_accumulate(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx,
                      const int64_t *idx, const double *kw, const double *dist, int64_t M,
                      double *sums, int32_t *status, void *ws, size_t ws_bytes, hipStream_t s);
// the same with the sample kernel computed on the fly (kw_i = 1 - sqrt(1 - exp(-gamma dist_i^2)),
// the arithmetic of dbgsom_exp_similarity) and the status flag also left as a float64 behind the
// sums (sums[M (d + 3)]: it rides in the all-reduce buffer): two launches less per epoch
int launch_accumulate_epoch(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx,
                            const int64_t *idx, double gamma, const double *dist, int64_t M,
                            double *sums, int32_t *status, void *ws, size_t ws_bytes, hipStream_t s);
// weighted forms (`sw`: one finite weight >= 0 per row; a row of weight w counts as w copies): factor
// sw kw on S and K, sw dist on E, a = sum sw as an ordered float64 sum; rows of weight 0 are not streamed
size_t accumulate_weighted_workspace_bytes(int64_t N, int64_t d, int64_t M);
int launch_accumulate_weighted(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx,
                               const int64_t *idx, const double *kw, const double *sw, const double *dist, int64_t M,
                               double *sums, int32_t *status, void *ws, size_t ws_bytes, hipStream_t s);
int launch_accumulate_epoch_weighted(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx,
                                     const int64_t *idx, double gamma, const double *sw, const double *dist, int64_t M,
                                     double *sums, int32_t *status, void *ws, size_t ws_bytes, hipStream_t s);
// CSR samples (csr.hip): canonical CSR on the device -- indptr int64 (N + 1), indices int32 strictly ascending
// within a row, data float32 / float64.  The search reads Wt (d x ldwt, ldwt = csr_wt_ld(M)), the transposed
// float64 prototypes; the sums go through the dense pipeline of accumulate.hip with the chunk kernel replaced.
struct CsrView {
    const int64_t *indptr = nullptr;
    const int32_t *indices = nullptr;
    const void *data = nullptr;
};
int64_t csr_wt_ld(int64_t M);
int launch_csr_row_sqnorms(const CsrView &x, int dtype, int64_t N, double *out, hipStream_t s);
int launch_transpose_weights(const double *W, int64_t M, int64_t d, int64_t ldw, double *Wt, int64_t ldwt,
                             hipStream_t s);
int launch_bmu_csr(const CsrView &x, int dtype, int64_t N, const double *xx, const double *Wt, int64_t ldwt,
                   int64_t M, const double *ww, int k, int round_f32, int64_t *idx, double *dist, hipStream_t s);
int launch_segsum_csr(const CsrView &x, int dtype, int64_t d, const int32_t *order, const double *kw, double gamma,
                      const double *dist, const uint32_t *seg_start, const uint32_t *count,
                      const uint32_t *chunk_pre, int64_t M, double *slab, const double *sw, int64_t maxchunks,
                      hipStream_t s);
int launch_csr_densify(const CsrView &x, int dtype, int64_t N, int64_t d, int64_t ld, void *out, hipStream_t s);
int launch_csr_rows_to_f64(const CsrView &x, int dtype, const int64_t *ids, int64_t n, int64_t cols, double *dst,
                           hipStream_t s);
// the sums of launch_accumulate* for CSR samples (kw == nullptr: the sample kernel with `gamma` on the fly and the
// status flag behind the sums, as launch_accumulate_epoch; sw != nullptr: the weighted form and its workspace)
int launch_accumulate_csr(const CsrView &x, int x_dtype, int64_t N, int64_t d, const int64_t *idx, const double *kw,
                          double gamma, const double *sw, const double *dist, int64_t M, double *sums,
                          int32_t *status, bool status_behind_sums, void *ws, size_t ws_bytes, hipStream_t s);
// rows with missing entries (masked.hip): NaN marks a hole, F32 / F64 rows; the search reads the transposed float64
// prototypes launch_masked_weights leaves in front of the workspace (one transposition serves many row chunks)
size_t bmu_masked_workspace_bytes(int x_dtype, int64_t N, int64_t d, int64_t M);
int masked_check_shape(int x_dtype, int64_t N, int64_t d, int64_t ldx, int64_t M, int k);
int launch_masked_weights(const double *W, int64_t M, int64_t d, int64_t ldw, void *ws, hipStream_t s);
int launch_bmu_masked_rows(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, int64_t M, int k,
                           int64_t *idx, double *dist, void *ws, size_t ws_bytes, hipStream_t s);
int launch_fill_missing(void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *W, int64_t M,
                        int64_t ldw, const int64_t *idx, int64_t idx_stride, hipStream_t s);
// the halves of launch_bmu_masked_rows for rows that stay resident: n_obs and the float64 copy of float32 rows (N x d)
// once, then any number of searches of the float64 rows X64 (ld64 apart) against Wt (masked_weights_bytes(d, M))
int launch_masked_prepare(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, int32_t *nobs, double *Xw,
                          hipStream_t s);
int launch_bmu_masked_prepared(const double *X64, int64_t N, int64_t d, int64_t ld64, const int32_t *nobs,
                               const double *Wt, int64_t M, int k, int64_t *idx, double *dist, hipStream_t s);
size_t masked_weights_bytes(int64_t d, int64_t M);
// the N x M distance matrix (distances.hip): dense rows (the chain of launch_bmu, every pair stored; rows ldo >= M
// apart) and rows with missing entries (the chain of launch_bmu_masked_rows, same workspace, Wt in front of it)
int launch_distances(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx, const double *W,
                     int64_t M, const double *ww, double *out, int64_t ldo, hipStream_t s);
int launch_distances_masked_rows(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, int64_t M, double *out,
                                 int64_t ldo, void *ws, size_t ws_bytes, hipStream_t s);
// the same storing the clamped squared value instead of its square root, with ordinary stores (the slab of
// kneighbors.hip, read back at once)
int launch_distances_squared(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx,
                             const double *W, int64_t M, const double *ww, double *out, int64_t ldo, hipStream_t s);
int launch_distances_masked_rows_squared(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, int64_t M,
                                         double *out, int64_t ldo, void *ws, size_t ws_bytes, hipStream_t s);
// the k nearest prototypes of every row (kneighbors.hip): the selection on a matrix of squared values, and the driver
// over slabs of rows (squared distances into the workspace, selection on the slab; slab_rows 0 = the default)
int launch_topk_rows(const double *R, int64_t N, int64_t M, int64_t ldr, int k, int64_t *idx, double *dist,
                     hipStream_t s);
int launch_topk_rows_plain(const double *R, int64_t N, int64_t M, int64_t ldr, int k, int64_t *idx, double *dist,
                           hipStream_t s);   // (no square root behind the selection: R holds distances)
// row_neighbors.hip: the k nearest rows of X to every query among the rows filed under its probed units (`fn`: the
// exported call the argument errors are reported under)
int launch_scan_cells(const char *fn, const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const int32_t *order,
                      const uint32_t *seg_start, int64_t M, const void *Q, int q_dtype, int64_t Nq, int64_t ldq,
                      const int64_t *probe, int n_probe, int k, int64_t *idx, double *dist, hipStream_t s);
int scan_cells_check(const char *fn, int x_dtype, int64_t N, int64_t d, int64_t ldx, int64_t M, int q_dtype, int64_t Nq,
                     int64_t ldq, int n_probe, int k);
int64_t kneighbors_slab_rows(int64_t N, int64_t M, int64_t slab_rows);
// rows of a slab are M rounded up to even apart, so that every row starts on 16 bytes
inline int64_t kneighbors_slab_ld(int64_t M) { return M + (M & 1); }
size_t kneighbors_workspace_bytes(int64_t N, int64_t M, int64_t slab_rows);
// the workspace of a slab loop under the name `fn` of its entry: `beside` bytes and the slab fit, then 16-byte alignment
static inline int kneighbors_workspace_check(const char *fn, int64_t N, int64_t M, int64_t slab_rows, const void *ws,
                                             size_t ws_bytes, size_t beside) {
    TRY_STATUS(workspace_check(fn, ws_bytes, beside + kneighbors_workspace_bytes(N, M, slab_rows)));
    if (!is_aligned(ws, 16)) {
        set_error("%s: workspace_dev must be 16-byte aligned", fn);
        return DBGSOM_EINVAL;
    }
    return DBGSOM_OK;
}
// The Euclidean slab loop (launch_kneighbors and everything else that reads a slab of squared distances back at once):
// the rows in slabs of kneighbors_slab_rows, launch_distances_squared of a slab's n rows from r0 on into `slab`, rows
// kneighbors_slab_ld(M) apart, then consume(r0, n, slab, ldr) on the same stream; the first non-zero status ends it.
template <typename Consume>
int euclidean_slabs(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx, const double *W,
                    int64_t M, const double *ww, int64_t slab_rows, double *slab, hipStream_t s, Consume consume) {
    const int64_t rows = kneighbors_slab_rows(N, M, slab_rows), ldr = kneighbors_slab_ld(M);
    const size_t es = dtype_size(x_dtype);
    for (int64_t r0 = 0; r0 < N; r0 += rows) {
        const int64_t n = rows < N - r0 ? rows : N - r0;
        TRY_STATUS(launch_distances_squared(static_cast<const char *>(X) + (size_t)r0 * ldx * es, x_dtype, n, d, ldx,
                                            xx + r0, W, M, ww, slab, ldr, s));
        TRY_STATUS(consume(r0, n, slab, ldr));
    }
    return DBGSOM_OK;
}
// The slab loop of the kneighbors launchers of the other forms (masked, Manhattan, cosine): fill(rows, r0, n, slab, ldr)
// stores what is selected on for the n rows from r0 on (`rows`: the first of them) into `slab`, rows ldr apart, then
// `select` (launch_topk_rows: the slab holds squared values; launch_topk_rows_plain: what is reported) on the slab.
template <typename Fill>
int kneighbors_slabs(const void *X, int x_dtype, int64_t N, int64_t ldx, int64_t M, int k, int64_t slab_rows, double *slab,
                     decltype(launch_topk_rows) *select, int64_t *idx, double *dist, hipStream_t s, Fill fill) {
    const int64_t rows = kneighbors_slab_rows(N, M, slab_rows), ldr = kneighbors_slab_ld(M);
    const size_t es = dtype_size(x_dtype);
    for (int64_t r0 = 0; r0 < N; r0 += rows) {
        const int64_t n = rows < N - r0 ? rows : N - r0;
        TRY_STATUS(fill(static_cast<const char *>(X) + (size_t)r0 * ldx * es, r0, n, slab, ldr));
        TRY_STATUS(select(slab, n, M, ldr, k, idx + r0 * k, dist + r0 * k, s));
    }
    return DBGSOM_OK;
}
size_t kneighbors_masked_workspace_bytes(int x_dtype, int64_t N, int64_t d, int64_t M, int64_t slab_rows);
int launch_kneighbors(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx, const double *W,
                      int64_t M, const double *ww, int k, int64_t slab_rows, int64_t *idx, double *dist, void *ws,
                      size_t ws_bytes, hipStream_t s);
int launch_kneighbors_masked_rows(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, int64_t M, int k,
                                  int64_t slab_rows, int64_t *idx, double *dist, void *ws, size_t ws_bytes,
                                  hipStream_t s);
// the distortion measure of every row (distortion.hip): b = the row's best matching unit, e = sum_j H[b, j] r_j, on a
// matrix of squared values, and the driver over slabs of rows (the slabs and the workspace of launch_kneighbors)
int launch_energy_rows(const double *R, int64_t N, int64_t M, int64_t ldr, const double *H, int64_t ldh, int64_t *bmu,
                       double *e, hipStream_t s);
int launch_neighborhood_energy(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx,
                               const double *W, int64_t M, const double *ww, const double *H, int64_t ldh,
                               int64_t slab_rows, int64_t *bmu, double *e, void *ws, size_t ws_bytes, hipStream_t s);
// the map as a Gaussian mixture (mixture.hip): per row the unit of the largest t_j = a_j - c r_j, lse = log sum_j exp(t_j)
// and q_v = sum_j exp(t_j) Y[j, v] / sum_j exp(t_j), on a matrix of squared values, and the driver over slabs of rows
// (the slabs and the workspace of launch_kneighbors); n_values == 0: Y and q are null
int launch_mixture_rows(const double *R, int64_t N, int64_t M, int64_t ldr, const double *a, double c, const double *Y,
                        int n_values, int64_t ldy, int64_t *unit, double *lse, double *q, int64_t ldq, hipStream_t s);
int launch_mixture(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx, const double *W, int64_t M,
                   const double *ww, const double *a, double c, const double *Y, int n_values, int64_t ldy, int64_t slab_rows,
                   int64_t *unit, double *lse, double *q, int64_t ldq, void *ws, size_t ws_bytes, hipStream_t s);
// the k nearest rows to every prototype (exemplars.hip): the fold down the columns of a matrix of squared values --
// state_r / state_i (M x k) hold per column the k smallest (r, global row) so far --, the slab loop of launch_kneighbors
// with that fold behind the product (rows row0 .. row0 + N - 1 into a caller's state), the kernel that stores the state
// as (sqrt(r), row), and the whole call with the state behind its workspace
size_t topk_cols_workspace_bytes(int64_t N, int64_t M, int k);
int launch_topk_cols_init(double *state_r, int64_t *state_i, int64_t M, int k, hipStream_t s);
int launch_topk_cols(const double *R, int64_t N, int64_t M, int64_t ldr, const int64_t *owner, int64_t row0, int k,
                     double *state_r, int64_t *state_i, void *ws, size_t ws_bytes, hipStream_t s);
size_t exemplars_fold_workspace_bytes(int64_t N, int64_t M, int k, int64_t slab_rows);
size_t exemplars_workspace_bytes(int64_t N, int64_t M, int k, int64_t slab_rows);
int launch_exemplars_fold(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx, const double *W,
                          int64_t M, const double *ww, int k, int own_cell, int64_t slab_rows, int64_t row0, double *state_r,
                          int64_t *state_i, void *ws, size_t ws_bytes, hipStream_t s);
int launch_exemplars_store(const double *state_r, const int64_t *state_i, int64_t M, int k, int64_t *idx, double *dist,
                           hipStream_t s);
int launch_exemplars(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx, const double *W,
                     int64_t M, const double *ww, int k, int own_cell, int64_t slab_rows, int64_t *idx, double *dist,
                     void *ws, size_t ws_bytes, hipStream_t s);
// the rows within a radius of every prototype (density.hip): the fold down the columns of a matrix of squared values --
// counts (M x n_radii int64) += #{ i : r_ij <= thr[t] } --, the slab loop of launch_kneighbors with that fold behind the
// product (into a caller's counts, which it does not zero), and the whole call, which does
size_t range_counts_workspace_bytes(int64_t N, int64_t M, int64_t slab_rows);
int launch_range_count_cols(const double *R, int64_t N, int64_t M, int64_t ldr, const double *thr, int n_radii,
                            int64_t *counts, hipStream_t s);
int launch_range_counts_fold(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx, const double *W,
                             int64_t M, const double *ww, const double *thr, int n_radii, int64_t slab_rows, int64_t *counts,
                             void *ws, size_t ws_bytes, hipStream_t s);
int launch_range_counts(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx, const double *W,
                        int64_t M, const double *ww, const double *thr, int n_radii, int64_t slab_rows, int64_t *counts,
                        void *ws, size_t ws_bytes, hipStream_t s);
// weighted geodesics over the lattice and the combined error read off them (geodesics.hip).  `status` is a zeroed
// device word the kernels OR their findings into; geodesics_status reads it back (blocking) and names the call `what`
size_t geodesics_workspace_bytes(int64_t M, int64_t E);
int launch_edge_lengths(const double *W, int64_t M, int64_t d, int64_t ldw, const int32_t *edges, int64_t E, double *len,
                        uint32_t *status, hipStream_t s);
int launch_geodesic_rows(const int32_t *edges, const double *len, int64_t E, int64_t M, const int32_t *sources, int64_t S,
                         double *G, int64_t ldg, uint32_t *status, hipStream_t s);
int launch_combined_error_rows(const int64_t *idx2, const double *dist, int64_t ldd, int64_t N, const double *G, int64_t ldg,
                               int64_t M, double *e, uint32_t *status, hipStream_t s);
int geodesics_status(const char *what, uint32_t *status_dev, int64_t M, hipStream_t s);
// metric="manhattan" (manhattan.hip): sum_k |x_k - w_k| in float64, F32 / F64 rows; search, matrix and selection read
// the transposed float64 prototypes launch_manhattan_weights leaves in front of the workspace
size_t bmu_manhattan_workspace_bytes(int x_dtype, int64_t N, int64_t d, int64_t M);
int launch_manhattan_weights(const double *W, int64_t M, int64_t d, int64_t ldw, void *ws, hipStream_t s);
int launch_bmu_manhattan_rows(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, int64_t M, int k,
                              int64_t *idx, double *dist, void *ws, size_t ws_bytes, hipStream_t s);
int launch_distances_manhattan_rows(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, int64_t M, double *out,
                                    int64_t ldo, void *ws, size_t ws_bytes, hipStream_t s);
size_t kneighbors_manhattan_workspace_bytes(int x_dtype, int64_t N, int64_t d, int64_t M, int64_t slab_rows);
int kneighbors_manhattan_check(int x_dtype, int64_t N, int64_t d, int64_t ldx, int64_t M, int k, int64_t slab_rows);
int launch_kneighbors_manhattan_rows(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, int64_t M, int k,
                                     int64_t slab_rows, int64_t *idx, double *dist, void *ws, size_t ws_bytes,
                                     hipStream_t s);
// metric="cosine" (cosine.hip; the cosine forms of the kernels of bmu.hip, bmu_dma.hip, distances.hip): c = 1 - (a u) v
// clamped to [0, 2], a the chain of launch_bmu, u = inv(|x|^2), v = inv(|w|^2) from launch_inv_norms; F32 / F64 rows.
// The launchers take u where their Euclidean namesakes take xx and v where they take ww.
int launch_inv_norms(const double *sq, int64_t n, double *out, hipStream_t s);
int launch_bmu_cosine(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *u, const double *W,
                      int64_t M, const double *v, int k, int64_t *idx, double *dist, hipStream_t s);
int launch_distances_cosine(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *u, const double *W,
                            int64_t M, const double *v, double *out, int64_t ldo, hipStream_t s);
// (the slab form: ordinary stores, the prototypes split over blockIdx.y)
int launch_distances_cosine_slab(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *u,
                                 const double *W, int64_t M, const double *v, double *out, int64_t ldo, hipStream_t s);
int launch_kneighbors_cosine(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *u, const double *W,
                             int64_t M, const double *v, int k, int64_t slab_rows, int64_t *idx, double *dist, void *ws,
                             size_t ws_bytes, hipStream_t s);
// fit on rows with missing entries: sums [S (M x d) | K (M x d) | A (M x d) | a | E] over the observed entries
// (masked_fit.hip), and the smoothing with a denominator per (neuron, feature) (smooth.hip)
size_t accumulate_masked_workspace_bytes(int64_t N, int64_t d, int64_t M);
int launch_accumulate_masked(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const int64_t *idx,
                             const double *kw, const double *dist, int64_t M, double *sums, int32_t *status, void *ws,
                             size_t ws_bytes, hipStream_t s);
size_t smooth_masked_workspace_bytes(int64_t M, int64_t d);
int launch_smooth_masked(const double *sums, int64_t M, int64_t d, const float *hop, double sigma, const double *W_old,
                         double *W_new, double *change_total, void *ws, size_t ws_bytes, hipStream_t s);
void bucket_sort_tables(const void *ws, int64_t N, int64_t M, const uint32_t **count, const uint32_t **seg_start,
                        const uint32_t **chunk_pre);
int accumulate_chunk_rows();
size_t bucket_sort_workspace_bytes(int64_t N, int64_t M);
int launch_bucket_sort(const int64_t *idx, int64_t N, int64_t M, int32_t *order, void *ws,
                       hipStream_t s);
const uint32_t *bucket_sort_seg_start(const void *ws, int64_t N, int64_t M);
// per-unit sums of N x V float64 values over the stable bucket order, blocks of 128 list rows and a fold over the
// blocks, and the elementwise deviations from M x V centres (unit_sums.hip); arguments checked by the callers
size_t unit_sums_workspace_bytes(int64_t N, int64_t M, int V, bool weighted);
int launch_unit_sums(const int64_t *unit, const double *Z, int64_t ldz, const double *w, int64_t N, int64_t M, int V,
                     double *mass, double *sums, int64_t lds, void *ws, size_t ws_bytes, hipStream_t s);
int launch_unit_deviations(const int64_t *unit, const double *Y, int64_t ldy, int64_t N, const double *C, int64_t ldc,
                           int64_t M, int V, int mode, double *out, int64_t ldo, hipStream_t s);
// the filtered search with everything the engine may add to the public dbgsom_bmu_filtered call
// optional per-stage timing of dbgsom_bmu_filtered (bench / profiling): events on the caller's stream
struct StageTimer {
    bool enabled = false, valid = false;
    hipEvent_t ev[6] = {};
    bool created = false;
    void mark(int k, hipStream_t s) {
        if (!enabled) return;
        if (!created) { for (auto &e : ev) (void)hipEventCreate(&e); created = true; }
        (void)hipEventRecord(ev[k], s);
    }
    void destroy() {
        if (created) for (auto &e : ev) (void)hipEventDestroy(e);
        created = false; valid = false;
    }
};

// a second stream for launches that may overlap (per FilterAux, created on first use; if it cannot be
// created the work simply stays on the caller's stream)
struct SideStream {
    hipStream_t stream = nullptr, stream2 = nullptr;
    hipEvent_t forked = nullptr, joined = nullptr, joined2 = nullptr, mid = nullptr;
    hipEvent_t gap_fork = nullptr, gap_done = nullptr;   // the prototype gaps beside the seed pre-pass
    int state = 0;  // 0 untried, 1 ready, -1 unavailable
    int device = -1;
    bool ready() {
        int dev = -1;
        if (hipGetDevice(&dev) != hipSuccess) return false;
        if (state == 0) {
            device = dev;
            // (lowest priority: what runs here is off the critical path -- a few long chains beside the
            //  caller's stream -- and must not starve the short dependent kernels there: at equal priority the
            //  bucket sort between the refinement and the pair kernel took 0.5 ms instead of 0.06)
            int prio_low = 0, prio_high = 0;
            (void)hipDeviceGetStreamPriorityRange(&prio_low, &prio_high);
            state = (hipStreamCreateWithPriority(&stream, hipStreamNonBlocking, prio_low) == hipSuccess &&
                     hipStreamCreateWithPriority(&stream2, hipStreamNonBlocking, prio_low) == hipSuccess &&
                     hipEventCreateWithFlags(&forked, hipEventDisableTiming) == hipSuccess &&
                     hipEventCreateWithFlags(&joined, hipEventDisableTiming) == hipSuccess &&
                     hipEventCreateWithFlags(&joined2, hipEventDisableTiming) == hipSuccess &&
                     hipEventCreateWithFlags(&mid, hipEventDisableTiming) == hipSuccess &&
                     hipEventCreateWithFlags(&gap_fork, hipEventDisableTiming) == hipSuccess &&
                     hipEventCreateWithFlags(&gap_done, hipEventDisableTiming) == hipSuccess) ? 1 : -1;
        }
        return state == 1 && dev == device;  // (another device current than the one the streams live on: no fork)
    }
    void destroy() {
        if (state == 1) {
            (void)hipStreamDestroy(stream); (void)hipStreamDestroy(stream2);
            for (hipEvent_t e : {forked, joined, joined2, mid, gap_fork, gap_done}) (void)hipEventDestroy(e);
        }
        state = 0;
    }
};

struct FilterAux {
    StageTimer timer;
    SideStream side;
    void destroy() { timer.destroy(); side.destroy(); }
};
int filter_stage_ms(FilterAux &aux, double *ms5);   // [0] slice W + tables, [1] pre-pass, [2] bucket sort, [3] sweep, [4] exact stage

struct FilteredCall {
    const void *X = nullptr;
    int x_dtype = 0;
    int64_t N = 0, d = 0, ldx = 0;
    const double *xx = nullptr;
    const void *xplanes = nullptr;
    const double *W = nullptr;
    int64_t M = 0;
    const double *ww = nullptr;
    const int64_t *prev_idx = nullptr;
    const int32_t *order = nullptr;
    int seed_stride = 0, sweep_planes = 0, round_f32 = 0;
    int k = 1;   // nearest prototypes per sample: 1, or 2 (idx / dist then hold N x 2; the pruning form only)
    int64_t *idx = nullptr;
    double *dist = nullptr;
    void *ws = nullptr;
    size_t ws_bytes = 0;
    hipStream_t stream = nullptr;
    // hinted pruning bound (filter.hip 2c): the previous epoch's exact distances and how far each
    // prototype has moved since
    const double *hint_dist = nullptr, *hint_shift = nullptr;
    // per-sample refinement of the candidate lists (2d): 0 = off, else the longest list it should take
    int refine_rows = 0;
    // the stored rows when they are not what X points to (bfloat16 storage behind a float32 copy): the
    // pair kernel of the refinement streams these
    const void *X_store = nullptr;
    int store_dtype = -1;
    int64_t ld_store = 0;
    // > 0: the call waits for its candidate lists and, when they average more than this, returns
    // DBGSOM_LISTS_LONG without the exact stage (idx / dist untouched): an arm of the search policy that has
    // never run on this map may leave the whole map a candidate, and the exact stage over such lists costs
    // twice the all-pairs search the caller can run instead
    double guard_mean = 0.0;
    // Seeds from per-load anchor buckets (filter.hip 2e; prev_idx == nullptr, the pruning form): `anchors` are
    // n_anchors rows of the samples as float64 (n_anchors x d), anchor_of[i] the anchor sample i was grouped with
    // and `order` the samples bucketed by it -- all three functions of the samples alone.  The call finds the
    // nearest prototype of every anchor, seeds each sample with its anchor's and runs neither the seed pre-pass
    // nor the bucket sort.
    const double *anchors = nullptr;
    const int32_t *anchor_of = nullptr;
    int n_anchors = 0;
    // ... and the run table of those buckets (launch_anchor_runs, filter.hip 2f; a function of the samples alone as
    // well): the candidate lists then come from the anchors' distances, without a pass over the samples' plane
    const void *anchor_runs = nullptr;
    // Only the seed pre-pass and the bucket sort (how the anchor buckets are built: W = the anchors): the arg-min
    // of the pre-pass goes to seeds_out, the bucket order to order_out (N int32 each); idx / dist are not written
    int32_t *seeds_out = nullptr, *order_out = nullptr;
    // stage timer and side streams of the caller (a context's own); nullptr: this thread's
    FilterAux *aux = nullptr;
};
constexpr int DBGSOM_LISTS_LONG = 1000;   // (internal status of launch_bmu_filtered, never crosses the ABI)
int launch_bmu_filtered(const FilteredCall &call);
// the run table of anchor buckets (filter.hip 2f): per 128-sample workgroup of `order` its runs of equal anchor
size_t anchor_runs_bytes(int64_t N, int n_anchors);
int launch_anchor_runs(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx,
                       const double *anchors, int n_anchors, const int32_t *anchor_of, const int32_t *order, void *runs,
                       size_t runs_bytes, hipStream_t s);
size_t smooth_workspace_bytes(int64_t M, int64_t d);
int launch_smooth(const double *sums, int64_t M, int64_t d, const float *hop, double sigma,
                  int layout, const double *W_old, double *W_new, double *change_total, void *ws,
                  size_t ws_bytes, hipStream_t s, bool total_by_caller = false);
// The row changes |W_i - W'_i|_2 a smoothing launch left in its workspace (M values).  total_by_caller (above) and a
// null change_total of launch_rowchange_blocks: no launch forms their sum -- a later kernel of the caller's does, with
// change_total_tree (the epoch's pack_results_kernel: one launch less per epoch).
const double *smooth_rowchg(const void *ws, int64_t M, int64_t d);
// smoothing sharded over the ranks (smooth.hip): column blocks of cb = smooth_block_cols columns; one block
// of the reduce-scatter buffer = S block (M x cb) = smooth_block_elems values; [K | a | E | status] stay in `sums`
int64_t smooth_block_cols(int64_t d, int nranks);
int64_t smooth_block_elems(int64_t M, int64_t d, int nranks);
int launch_pack_blocks(const double *sums, int64_t M, int64_t d, int nranks, double *out, hipStream_t s);
int launch_smooth_block(const double *S_b, const double *K, const double *a, int64_t M, int64_t cb, int64_t d_full,
                        const float *hop, double sigma, int layout, double *Wb, void *ws, size_t ws_bytes,
                        hipStream_t s);
int launch_rowchange_blocks(const double *blocks, int64_t M, int64_t d, int64_t cb, const double *W_old, double *W_new,
                            double *change_total, void *ws, hipStream_t s);

}  // namespace dbgsom
