// Context-level C ABI (include/dbgsom_hip.h, "Context-level entry points"): the host engine of the
// batch-SOM hot path.  A context owns one GPU's share of the job -- the resident samples (padded,
// optionally bfloat16), their norms and int8 digit planes, the prototypes, every workspace -- and
// runs the epoch body of BaseSom._grow_som (reference dbgsom/BaseSom.py:403-407) as one blocking
// call.  What used to be Python policy lives here: feature padding, the choice between the
// all-pairs and the filtered BMU search ("auto" / back-off), the adaptive number of digit planes,
// previous winners as seeds, device-resident prototypes between epochs, the one all-reduce per
// epoch (through the caller's callback).  No kernels of the hot path in this file: it drives the
// launchers of bmu*.hip, filter.hip, accumulate.hip, smooth.hip, stats.hip, csr.hip (CSR residents).
#include <dlfcn.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <new>
#include <vector>

#include "anchor_chain.h"
#include "common.h"
#include "epoch_control.h"

namespace dbgsom {

// a device allocation that grows on demand and is reused across calls
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    // tight: allocate what is asked for, without the head room for a growing map (the buffers of a context whose
    // resident samples are CSR: such data is loaded because memory is short, and a growth step then pays a
    // reallocation of the buffers that scale with M)
    bool tight = false;
    int reserve(size_t bytes) {
        if (bytes <= cap) return DBGSOM_OK;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        const size_t want = tight ? align_up(bytes) : align_up(bytes + bytes / 8, 1 << 20);
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            p = nullptr;
            (void)hipGetLastError();
            set_error("hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
            return DBGSOM_ENOMEM;
        }
        cap = want;
        return DBGSOM_OK;
    }
    // (re)allocations come zero-filled: the "last workgroup" tickets at the front of the filter
    // workspace must be 0 before their first use (they reset themselves afterwards)
    int reserve_zeroed(size_t bytes, hipStream_t s) {
        if (bytes <= cap) return DBGSOM_OK;
        const int rc = reserve(bytes);
        if (rc != DBGSOM_OK) return rc;
        hipError_t e = hipMemsetAsync(p, 0, cap, s);
        if (e != hipSuccess) { set_error("hipMemsetAsync failed: %s", hipGetErrorString(e)); return DBGSOM_EHIP; }
        return DBGSOM_OK;
    }
    // grow and keep the first `keep` bytes (ordered on `s`)
    int reserve_keep(size_t bytes, size_t keep, hipStream_t s) {
        if (bytes <= cap) return DBGSOM_OK;
        void *old = p;
        const size_t old_cap = cap;
        p = nullptr;
        cap = 0;
        const int rc = reserve(bytes * 2);
        if (rc != DBGSOM_OK) { p = old; cap = old_cap; return rc; }
        if (old && keep) {
            hipError_t e = hipMemcpyAsync(p, old, keep, hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) { set_error("device copy failed: %s", hipGetErrorString(e)); (void)hipFree(old); return DBGSOM_EHIP; }
        }
        if (old) (void)hipFree(old);
        return DBGSOM_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};

// page-locked host staging for the small per-epoch results
struct PinBuf {
    void *p = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes) {
        if (bytes <= cap) return DBGSOM_OK;
        if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; }
        const size_t want = align_up(bytes * 2, 4096);
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocMapped);
        if (e == hipSuccess) e = hipHostGetDevicePointer(&dev, p, 0);
        if (e != hipSuccess) { if (p) (void)hipHostFree(p); p = nullptr; dev = nullptr; (void)hipGetLastError(); set_error("hipHostMalloc(%zu) failed: %s", want, hipGetErrorString(e)); return DBGSOM_ENOMEM; }
        cap = want;
        return DBGSOM_OK;
    }
    void *dev = nullptr;  // the same memory as the GPU addresses it (kernels write results straight into it)
    void release() { if (p) (void)hipHostFree(p); p = nullptr; dev = nullptr; cap = 0; }
    template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};

// ---- small helper kernels ----------------------------------------------------------------------
// float32 -> bfloat16 (round to nearest even, NaN stays NaN) and back: the rows that stay resident
// and the exactly widened copy the BMU kernels read
__global__ void round_bf16_kernel(float *__restrict__ x, uint16_t *__restrict__ out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t u = __float_as_uint(x[i]);
        uint16_t b;
        if ((u & 0x7fffffffu) > 0x7f800000u) b = 0x7fc0;
        else b = (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
        out[i] = b;
        x[i] = __uint_as_float(((uint32_t)b) << 16);
    }
}
__global__ void widen_bf16_kernel(const uint16_t *__restrict__ in, float *__restrict__ out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = __uint_as_float(((uint32_t)in[i]) << 16);
}
__global__ void f64_to_f32_kernel(const double *__restrict__ in, float *__restrict__ out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = (float)in[i];
}
__global__ void u64_to_f64_kernel(const unsigned long long *__restrict__ in, double *__restrict__ out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = (double)in[i];
}
// The epoch's small results in ONE kernel straight into page-locked host memory (no copy engine
// round trips behind the last kernel: four queued D2H copies cost ~30 us per epoch):
// out = [a (M) | E (M) | change_total | status | sum of candidate-list lengths | the same of a pruning probe |
//        workgroups of the pruning form with long lists | workgroups anchor_mark_kernel handed over (the lean form:
//        long lists it kept)]
// change_total is formed here, by the first workgroup, from the row changes the smoothing left (change_total_tree:
// the launch and the ticket the row-change kernel used to spend on it are gone).  Workgroups of 256 threads.
__global__ __launch_bounds__(256) void pack_results_kernel(const double *__restrict__ aE, int64_t M,
                                                           const double *__restrict__ rowchg,
                                                           const double *__restrict__ status,
                                                           const unsigned long long *__restrict__ list_sum,
                                                           double *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * M; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = aE[i];
    double chg = 0.0;
    if (blockIdx.x == 0) chg = change_total_tree(rowchg, (int)M);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        out[2 * M] = chg;
        out[2 * M + 1] = status[0];
        out[2 * M + 2] = list_sum ? (double)list_sum[0] : 0.0;
        out[2 * M + 3] = list_sum ? (double)list_sum[1] : 0.0;  // (of a counting-only pruning launch)
        out[2 * M + 4] = list_sum ? (double)list_sum[2] : 0.0;  // (workgroups whose pruned lists came out long)
        out[2 * M + 5] = list_sum ? (double)list_sum[3] : 0.0;  // (workgroups whose lists from the anchors came out long)
    }
    __threadfence_system();
}
// shift[p] >= |a_p - b_p| (Euclidean, rows of two M x ld matrices) for p < rows, +inf beyond: how far a
// prototype has moved since the distances of the hint were measured (filter.hip 2c); one wavefront per row
__global__ __launch_bounds__(64) void row_shift_kernel(const double *__restrict__ A, const double *__restrict__ B,
                                                       int64_t ld, int64_t d, int64_t rows, int64_t M,
                                                       double *__restrict__ shift) {
    const int64_t p = blockIdx.x;
    if (p >= M) return;
    if (p >= rows) { if (threadIdx.x == 0) shift[p] = INFINITY; return; }
    double acc = 0.0;
    if (A != B)
        for (int64_t k = threadIdx.x; k < d; k += 64) {
            const double t = A[p * ld + k] - B[p * ld + k];
            acc = fma(t, t, acc);
        }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    // (rounding of d squares and sums: relative d 2^-52 at most; NaN rows give NaN -- "no bound")
    if (threadIdx.x == 0) shift[p] = sqrt(acc) * (1.0 + 1e-9);
}
__global__ void status_to_f64_kernel(const int32_t *__restrict__ status, double *__restrict__ out) {
    out[0] = status[0] ? 1.0 : 0.0;
}
// rows of a (rows x ld) matrix of element size ES gathered by index, 16 bytes per thread where aligned
template <typename T>
__global__ void gather_rows_kernel(const T *__restrict__ src, int64_t ld, const int32_t *__restrict__ ids,
                                   int64_t first, int64_t n, int64_t cols, T *__restrict__ dst) {
    const int64_t r = blockIdx.x;
    if (r >= n) return;
    const T *s = src + (int64_t)ids[first + r] * ld;
    T *d = dst + r * cols;
    for (int64_t c = threadIdx.x; c < cols; c += blockDim.x) d[c] = s[c];
}
__global__ void gather_f64_kernel(const double *__restrict__ src, const int32_t *__restrict__ ids, int64_t first,
                                  int64_t n, double *__restrict__ dst) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = src[ids[first + i]];
}
__global__ void gather_i32_kernel(const int32_t *__restrict__ src, const int32_t *__restrict__ ids, int64_t first,
                                  int64_t n, int32_t *__restrict__ dst) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = src[ids[first + i]];
}
template <typename T>
__global__ void rows_to_f64_kernel(const T *__restrict__ src, int64_t ld, const int64_t *__restrict__ ids, int64_t n,
                                   int64_t cols, double *__restrict__ dst) {
    const int64_t r = blockIdx.x;
    if (r >= n) return;
    const T *s = src + ids[r] * ld;
    for (int64_t c = threadIdx.x; c < cols; c += blockDim.x) dst[r * cols + c] = widen(s[c]);
}
__global__ void iota_i32_kernel(int32_t *__restrict__ a, int32_t *__restrict__ b, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        a[i] = b[i] = (int32_t)i;
}
__global__ void seg_counts_kernel(const uint32_t *__restrict__ seg_start, int64_t M, int64_t N, int64_t *__restrict__ counts) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < M; j += (int64_t)gridDim.x * blockDim.x)
        counts[j] = (int64_t)((j + 1 < M ? seg_start[j + 1] : (uint32_t)N) - seg_start[j]);
}

static unsigned grid1d(int64_t n, int block = 256) {
    const int64_t nb = (n + block - 1) / block;
    return (unsigned)(nb < 1 ? 1 : (nb > 8192 ? 8192 : nb));
}

}  // namespace dbgsom

using namespace dbgsom;

// the device-level ABI the engine drives (defined in filter.hip / stats.hip)
extern "C" {
const unsigned long long *dbgsom_filter_count_sum_ptr(const void *workspace_dev, int64_t N, int64_t d, int64_t M);
size_t dbgsom_filter_planes_bytes(int64_t rows, int64_t d);
size_t dbgsom_bmu_filtered_workspace_bytes(int64_t N, int64_t d, int64_t M);
}

namespace {

struct Samples {  // one resident sample set (training samples, or a query batch)
    int dtype = -1;            // storage dtype in HBM
    int64_t N = 0, d = 0, dp = 0;
    const void *X = nullptr;   // N x dp, storage dtype (own.p or borrowed)
    const void *Xb = nullptr;  // what the BMU kernels read: X, or the float32 copy of bfloat16 rows
    int bdtype = -1;
    DevBuf own, x32, xx, planes;
    bool planes_ready = false;
    // Anchor buckets of the stateless pruning search (filter.hip 2e), built on first use and valid as long as the
    // planes are: n_anchors rows of X as float64 with their norms behind them, the anchor every row was grouped
    // with and the rows bucketed by it.  A function of X alone.  anchor_state: 0 none, 1 in use, 2 dropped (their
    // lists came out longer than the pre-pass's: the pre-pass seeds this sample set again)
    // anchor_runs: the run table of the bucket order (filter.hip 2f), built and dropped with the buckets
    DevBuf anchors, anchor_of, anchor_order, anchor_runs;
    int64_t n_anchors = 0;
    int anchor_state = 0;
    int64_t anchor_generation = 0;   // goes up whenever the buckets go (a load, a rebuild, the valve): LeanGate
    void drop_anchors(int state) {
        anchors.release(); anchor_of.release(); anchor_order.release(); anchor_runs.release();
        n_anchors = 0; anchor_state = state; ++anchor_generation;
    }
    void drop_planes() { planes_ready = false; drop_anchors(0); }
    // CSR residents (dbgsom_ctx_load_csr at or above "csr_densify_below" features): X stays nullptr, the rows are
    // the three arrays below; dtype F32 / F64, dp = pad16(d) as for dense rows (prototypes and sums keep their layout)
    bool csr = false;
    int64_t nnz = 0;
    DevBuf indptr, indices, data;
    CsrView view() const { return CsrView{indptr.as<int64_t>(), indices.as<int32_t>(), data.p}; }
    void release() {
        own.release(); x32.release(); xx.release(); planes.release(); indptr.release(); indices.release(); data.release();
        drop_planes(); csr = false; nnz = 0; dtype = -1; N = 0; X = Xb = nullptr;
    }
};

}  // namespace

struct dbgsom_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // options
    int timing = 0;
    bool last_refined = false;
    bool last_k2_filtered = false;  // the last k = 2 search went through the pruning form
    int64_t filter_min_query_rows = 32768;
    int64_t sc_chunk_rows = 32768;  // sparse coding: query rows per chunk
    int64_t sc_cap = 0;             // sparse coding: active-set cap of the LDS path (0 = library default)
    DevBuf sc_ws, sc_x, sc_w, sc_p, sc_code, sc_proba, sc_cnt;
    int64_t masked_chunk_rows = 32768;  // rows with missing entries: query rows per chunk
    DevBuf mk_ws, mk_x, mk_w, mk_idx, mk_dist;
    // the distance matrix of a query (distances.hip): rows per chunk of the host-facing calls (0: as many as keep a
    // chunk's staged result at 256 MiB) and the staged result of a chunk
    int64_t distances_chunk_rows = 0;
    DevBuf pd_out;
    // the k nearest prototypes of a query (kneighbors.hip): rows per slab of squared distances (0: as many as keep
    // the slab at 64 MiB), the slab (masked rows: the masked search's workspace in front of it) and a chunk's result
    int64_t kneighbors_slab_rows = 0;
    DevBuf kn_ws, kn_idx, kn_dist;
    // the distortion measure of a query (distortion.hip): the M x M neighbourhood factors of the call (the slab and a
    // chunk's staged result are kn_ws, kn_idx and kn_dist); the mixture of a query (mixture.hip): [the log-priors | Y] of
    // the call (its third result is staged in pd_out)
    DevBuf de_h;
    // the combined error of a query (geodesics.hip): the M x M geodesics of the call, and the edges, their lengths and
    // the status word in front of a chunk's distances (the pairs and e are staged in kn_idx / kn_dist)
    DevBuf ce_g, ce_ws;
    // the k nearest rows to every prototype (exemplars.hip): the state of the call's fold, [r: M x k float64 | i: M x k
    // int64] (the slab and the fold's scratch are kn_ws; a host-facing call's result is staged in kn_idx and kn_dist)
    DevBuf ex_state;
    // the rows within a radius of every prototype (density.hip): the state of the call's fold, [counts: M x n_radii int64
    // | the thresholds: n_radii float64] (the slab is kn_ws; the counts come down from here, nothing is staged)
    DevBuf rc_state;
    // The resident rows have missing entries (NaN): option "incomplete", set after a load and cleared by the next one.
    // What depends on the rows alone is made when the option is set, once per load: n_obs per row (mf_nobs) and, for
    // float32 rows, their float64 copy (mf_x64, N x d x 8 bytes of HBM).  The ordinary calls then refuse to compute
    // on the rows; dbgsom_ctx_bmu_masked / dbgsom_ctx_epoch_masked take their place (prototypes M x d, unpadded,
    // handed over with every call).
    bool incomplete = false;
    DevBuf mf_nobs, mf_x64, mf_wt, mf_w, mf_wn, mf_idx, mf_dist, mf_kw, mf_sums, mf_acc_ws, mf_sm_ws, mf_scal;
    // metric="manhattan" (manhattan.hip): the workspace of the search of the resident rows (the transposed prototypes
    // and, for float32 rows, their float64 copy; its contents are made per call, the allocation is kept between the
    // epochs of a fit and goes with the context, counted in "device_bytes" like every buffer of CTX_DEVBUFS)
    DevBuf l1_ws;
    // metric="cosine" (cosine.hip): u = inv(|x|^2) of the resident rows, made once per load from their resident norms
    // (cos_u_ready), and [|w|^2 | v] of the prototypes of the call; both go with the context, counted in "device_bytes"
    DevBuf cos_u, cos_v;
    bool cos_u_ready = false;
    // samples
    Samples xs, xq;
    DevBuf y;
    bool has_labels = false;
    // one float64 weight per resident row (dbgsom_ctx_set_sample_weight): the epoch, dbgsom_ctx_update and the
    // reductions then run their weighted forms
    DevBuf sw, wh_order, wh_ws;
    bool has_weights = false;
    // float64 targets of the resident rows (dbgsom_ctx_set_targets: N x target_V, contiguous), and the buffers of the
    // per-unit sums (unit_sums.hip): workspace, staged host inputs, the small per-unit results, per-row deviations
    DevBuf ty, us_ws, us_in, us_out, us_dev;
    bool has_targets = false;
    int target_V = 0;
    // topology
    int64_t topoM = 0;
    DevBuf hop, hop_stage;
    // prototypes: two M x dp float64 buffers
    DevBuf Wb[2];
    int cur = 0;
    int64_t M = 0;       // rows of the resident prototypes (Wb[cur])
    int64_t otherM = 0;  // rows of Wb[cur ^ 1]
    // per-epoch device state
    DevBuf ww, idx[2], dist, kw, sums, acc_ws, sm_ws, filt_ws, scal, qidx, qdist, red, hist, stage_dev;
    // CSR residents: the transposed float64 prototypes the CSR search reads (rebuilt from Wb[cur] in front of every
    // search), and the feature count below which dbgsom_ctx_load_csr expands into dense rows (0 = never)
    DevBuf wt;
    int64_t csr_densify_below = 1024;
    int icur = 0;            // idx[icur]: winners of the last epoch (the hint)
    ResidentSearchState search;   // what the last search left in idx[icur], `dist` and the bucket order (epoch_control.h)
    int64_t sumsM = 0;
    // partition (vertical growth)
    DevBuf part_order, part_ws, part_counts;
    int64_t partM = 0;
    bool part_valid = false;
    // which form of the filtered search runs next, and what it has learnt (search_policy.h)
    SearchPolicy policy;
    DevBuf shiftb;   // the prototypes' shifts of the hinted pruning bound (filter.hip 2c)
    // last epoch
    bool last_filtered = false;
    int64_t last_filter_M = 0, last_filter_N = 0, last_filter_d = 0;
    const void *last_filter_ws = nullptr;
    // staging
    PinBuf tail, counts;
    // collective: the caller's callback, or RCCL driven from here
    dbgsom_allreduce_fn allreduce = nullptr;
    void *allreduce_user = nullptr;
    void *rccl_comm = nullptr;
    bool rccl_owned = false;
    // smoothing sharded over the ranks (columns of W'): the epoch's collective is then a reduce-scatter of column
    // blocks of the sums and an all-gather of the W' blocks (smooth.hip).  shard_smooth: 0 = never, 1 = whenever
    // the collective can do it, 2 = when the smoothing GEMM is large (default).  Needs rank / nranks: from the
    // RCCL communicator, or from dbgsom_ctx_set_collectives.
    dbgsom_collective_fn coll = nullptr;
    void *coll_user = nullptr;
    int coll_rank = 0, coll_nranks = 1;
    int shard_smooth = 2;
    bool sums_sharded = false;   // the last accumulate step left the reduced sums as this rank's block
    int64_t shard_epochs = 0;    // epochs smoothed that way (diagnostics)
    DevBuf shard_send, shard_gather;
    // traffic of the prototypes across PCIe (f-4 evidence: whole matrices only at the first epoch, at
    // growth steps and at the end of a fit)
    int64_t w_up_calls = 0, w_up_bytes = 0, w_down_calls = 0, w_down_bytes = 0, w_row_writes = 0, w_row_reads = 0;
    // traffic of the samples across PCIe: rows host -> HBM (loads, query placements, the chunks of the coder and of
    // the masked search) and per-row results HBM -> host (winners, distances, codes, probabilities, filled rows).
    // Rows that are in HBM already (dbgsom_ctx_load_device, the *_device queries) move neither.
    int64_t x_up_bytes = 0, x_up_calls = 0, x_down_bytes = 0;
    void x_up(size_t bytes) { x_up_bytes += (int64_t)bytes; ++x_up_calls; }
    void x_down(size_t bytes) { x_down_bytes += (int64_t)bytes; }
    // timing
    hipEvent_t ev[4] = {};
    bool ev_created = false, ev_valid = false;
    double filter_ms[5] = {0, 0, 0, 0, 0};
    bool filter_ms_valid = false;
    FilterAux faux;   // this context's stage timer and side streams of the filtered search (FilteredCall::aux)
    // anchor buckets seed the stateless pruning search of the resident samples ("anchor_seeds", default on)
    int anchor_seeds = 1;
    // buckets built / searches seeded from them / epochs that took the lean form of such a search so far
    int64_t anchor_builds = 0, anchor_searches = 0, lean_searches = 0;
    int64_t hint_bound_searches = 0;   // searches that took the hinted pruning bound (plan.hint_bound)
    AnchorControl anchor;   // when the anchors seed a search, in which form, and the valve (epoch_control.h)
};

namespace {

#define CTX_CHECK(c)                                                                 \
    do {                                                                             \
        if (!(c)) { set_error("%s: null context", __func__); return DBGSOM_EINVAL; } \
        DBGSOM_HIP_CHECK(hipSetDevice((c)->device));                                 \
    } while (0)
#define TRY(expr) do { int _rc = (expr); if (_rc != DBGSOM_OK) return _rc; } while (0)

inline int64_t pad16(int64_t d) { return (d + 15) / 16 * 16; }

int sync(dbgsom_ctx *c) {
    DBGSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
    return DBGSOM_OK;
}

// host (rows x d, element size es) -> device (rows x dp), zeros behind column d
int upload_padded(dbgsom_ctx *c, void *dst, const void *src, int64_t rows, int64_t d, int64_t dp, size_t es) {
    if (rows == 0) return DBGSOM_OK;
    if (d == dp) {
        DBGSOM_HIP_CHECK(hipMemcpyAsync(dst, src, (size_t)rows * d * es, hipMemcpyHostToDevice, c->stream));
    } else {
        DBGSOM_HIP_CHECK(hipMemsetAsync(dst, 0, (size_t)rows * dp * es, c->stream));
        DBGSOM_HIP_CHECK(hipMemcpy2DAsync(dst, (size_t)dp * es, src, (size_t)d * es, (size_t)d * es, (size_t)rows,
                                          hipMemcpyHostToDevice, c->stream));
    }
    return DBGSOM_OK;
}

int download_unpadded(dbgsom_ctx *c, void *dst, const void *src, int64_t rows, int64_t d, int64_t dp, size_t es) {
    if (rows == 0) return DBGSOM_OK;
    if (d == dp)
        DBGSOM_HIP_CHECK(hipMemcpyAsync(dst, src, (size_t)rows * d * es, hipMemcpyDeviceToHost, c->stream));
    else
        DBGSOM_HIP_CHECK(hipMemcpy2DAsync(dst, (size_t)d * es, src, (size_t)dp * es, (size_t)d * es, (size_t)rows,
                                          hipMemcpyDeviceToHost, c->stream));
    return DBGSOM_OK;
}

// norms + BMU view of a freshly placed sample set (s.X, s.dtype, s.N, s.d, s.dp set)
int finish_samples(dbgsom_ctx *c, Samples &s, bool x32_is_widened) {
    if (s.dtype == DBGSOM_BF16) {
        if (!x32_is_widened) {
            TRY(s.x32.reserve((size_t)s.N * s.dp * 4));
            hipLaunchKernelGGL(widen_bf16_kernel, dim3(grid1d(s.N * s.dp)), dim3(256), 0, c->stream,
                               (const uint16_t *)s.X, s.x32.as<float>(), s.N * s.dp);
            TRY(launch_status("widen_bf16_kernel"));
        }
        s.Xb = s.x32.p;
        s.bdtype = DBGSOM_F32;
    } else {
        s.Xb = s.X;
        s.bdtype = s.dtype;
    }
    TRY(s.xx.reserve((size_t)s.N * 8));
    TRY(launch_row_sqnorms(s.Xb, s.bdtype, s.N, s.dp, s.dp, s.xx.as<double>(), c->stream));
    s.drop_planes();
    return DBGSOM_OK;
}

int place_host_samples(dbgsom_ctx *c, Samples &s, const void *X_host, int x_dtype, int64_t N, int64_t d, int storage) {
    DBGSOM_REQUIRE(valid_dtype(x_dtype) && valid_dtype(storage), "dtype must be DBGSOM_F32/F64/BF16");
    DBGSOM_REQUIRE(X_host && N >= 1 && d >= 1 && N < 0x7fffffff, "bad samples");
    DBGSOM_REQUIRE(storage == x_dtype || (storage == DBGSOM_BF16 && x_dtype == DBGSOM_F32),
                   "storage must be the input dtype, or DBGSOM_BF16 for float32 input");
    const int64_t dp = pad16(d);
    s.N = N; s.d = d; s.dp = dp; s.dtype = storage;
    s.csr = false; s.nnz = 0;
    bool widened = false;
    if (storage == DBGSOM_BF16 && x_dtype == DBGSOM_F32) {
        TRY(s.x32.reserve((size_t)N * dp * 4));
        TRY(s.own.reserve((size_t)N * dp * 2));
        TRY(upload_padded(c, s.x32.p, X_host, N, d, dp, 4));
        hipLaunchKernelGGL(round_bf16_kernel, dim3(grid1d(N * dp)), dim3(256), 0, c->stream, s.x32.as<float>(),
                           s.own.as<uint16_t>(), N * dp);
        TRY(launch_status("round_bf16_kernel"));
        widened = true;
    } else {
        const size_t es = dtype_size(x_dtype);
        TRY(s.own.reserve((size_t)N * dp * es));
        TRY(upload_padded(c, s.own.p, X_host, N, d, dp, es));
    }
    s.X = s.own.p;
    c->x_up((size_t)N * d * dtype_size(x_dtype));
    return finish_samples(c, s, widened);
}

// rows that already live in HBM on the context's device (ldx elements apart): borrowed when they are what the kernels
// want -- rows of a multiple of 16 features, contiguous, 16-byte aligned --, else copied (padded) into s.own on the
// device.  A borrowed s.X is the caller's memory: whoever places a query this way clears it before returning.
bool device_rows_conform(const void *X_dev, int64_t d, int64_t ldx) {
    return ldx == pad16(d) && d == ldx && is_aligned(X_dev, 16);
}

int place_device_samples(dbgsom_ctx *c, Samples &s, const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx) {
    DBGSOM_REQUIRE(valid_dtype(x_dtype), "x_dtype must be DBGSOM_F32/F64/BF16");
    DBGSOM_REQUIRE(X_dev && N >= 1 && d >= 1 && ldx >= d && N < 0x7fffffff, "bad samples");
    const size_t es = dtype_size(x_dtype);
    const int64_t dp = pad16(d);
    s.dtype = -1;
    s.N = N; s.d = d; s.dp = dp;
    s.csr = false; s.nnz = 0;
    s.indptr.release(); s.indices.release(); s.data.release();
    if (device_rows_conform(X_dev, d, ldx)) {
        s.own.release();
        s.X = X_dev;  // borrowed
    } else {
        TRY(s.own.reserve((size_t)N * dp * es));
        if (d != dp) DBGSOM_HIP_CHECK(hipMemsetAsync(s.own.p, 0, (size_t)N * dp * es, c->stream));
        DBGSOM_HIP_CHECK(hipMemcpy2DAsync(s.own.p, (size_t)dp * es, X_dev, (size_t)ldx * es, (size_t)d * es, (size_t)N,
                                          hipMemcpyDeviceToDevice, c->stream));
        s.X = s.own.p;
    }
    s.dtype = x_dtype;
    return finish_samples(c, s, false);
}

// The rows of a query: a host pointer (Nq x d, contiguous) or a device pointer (rows ldx elements apart).
struct QueryRows {
    const void *p;
    bool on_device;
    int64_t ldx;
};

int place_query_rows(dbgsom_ctx *c, Samples &s, const QueryRows &q, int x_dtype, int64_t Nq, int64_t d) {
    if (q.on_device) return place_device_samples(c, s, q.p, x_dtype, Nq, d, q.ldx);
    return place_host_samples(c, s, q.p, x_dtype, Nq, d, x_dtype);
}

// after a query: nothing of the caller's stays referenced, and a large one-off batch is not sat on
void drop_query_rows(Samples &s, const QueryRows &q, int64_t held_bytes) {
    if (q.on_device && s.X != s.own.p) { s.X = s.Xb = nullptr; s.dtype = -1; s.drop_planes(); }
    if (held_bytes > ((int64_t)256 << 20)) s.release();
}

int ensure_planes(dbgsom_ctx *c, Samples &s) {
    if (s.planes_ready) return DBGSOM_OK;
    const size_t nbytes = dbgsom_filter_planes_bytes(s.N, s.dp);
    TRY(s.planes.reserve(nbytes));
    TRY(dbgsom_filter_prepare(s.Xb, s.bdtype, s.N, s.dp, s.dp, s.planes.p, s.planes.cap, c->stream));
    s.planes_ready = true;
    return DBGSOM_OK;
}

// The anchor buckets of a dense sample set (filter.hip 2e), once per load: A = min(256, N) anchors, rows
// floor(k N / A) of X; every sample goes to its nearest anchor by the seed pre-pass run against the anchors as if
// they were a map of A prototypes (every anchor, every feature: about four of an epoch's pre-passes), and the bucket
// sort behind it leaves the samples grouped by anchor.  N < 256: every row is its own anchor.
// The anchors are numbered along a greedy nearest-neighbour chain (anchor_chain.h: anchor_rows, chain_anchors).
// rows `rows` of the samples as float64 (rows.size() x dp), waited for
int gather_anchor_rows(dbgsom_ctx *c, Samples &s, const std::vector<int64_t> &rows, double *anchors) {
    const int64_t A = (int64_t)rows.size(), dp = s.dp;
    TRY(c->stage_dev.reserve((size_t)A * 8));
    int64_t *ids = c->stage_dev.as<int64_t>();
    DBGSOM_HIP_CHECK(hipMemcpyAsync(ids, rows.data(), (size_t)A * 8, hipMemcpyHostToDevice, c->stream));
    DBGSOM_HIP_CHECK(hipStreamSynchronize(c->stream));   // (pageable memory: the caller's vector may go)
    if (s.dtype == DBGSOM_F32)
        hipLaunchKernelGGL(rows_to_f64_kernel<float>, dim3((unsigned)A), dim3(256), 0, c->stream, (const float *)s.X, dp, ids, A, dp, anchors);
    else if (s.dtype == DBGSOM_F64)
        hipLaunchKernelGGL(rows_to_f64_kernel<double>, dim3((unsigned)A), dim3(256), 0, c->stream, (const double *)s.X, dp, ids, A, dp, anchors);
    else
        hipLaunchKernelGGL(rows_to_f64_kernel<bf16_t>, dim3((unsigned)A), dim3(256), 0, c->stream, (const bf16_t *)s.X, dp, ids, A, dp, anchors);
    TRY(launch_status("rows_to_f64_kernel"));
    return DBGSOM_OK;
}

// a filtered search of the samples `s` under the M x s.dp prototypes W (norms ww) on the context's stream
FilteredCall filtered_call(dbgsom_ctx *c, Samples &s, const double *W, int64_t M, const double *ww) {
    FilteredCall call;
    call.aux = &c->faux;
    call.X = s.Xb; call.x_dtype = s.bdtype; call.N = s.N; call.d = s.dp; call.ldx = s.dp;
    call.xx = s.xx.as<double>(); call.xplanes = s.planes.p; call.W = W; call.M = M; call.ww = ww;
    call.stream = c->stream;
    return call;
}

int ensure_anchors(dbgsom_ctx *c, Samples &s) {
    if (s.anchor_state != 0) return DBGSOM_OK;
    TRY(ensure_planes(c, s));
    const int64_t A = s.N < 256 ? s.N : 256, dp = s.dp;
    TRY(s.anchors.reserve((size_t)A * dp * 8 + (size_t)A * 8));
    TRY(s.anchor_of.reserve((size_t)s.N * 4));
    TRY(s.anchor_order.reserve((size_t)s.N * 4));
    std::vector<int64_t> rows = anchor_rows(s.N, A);
    double *anchors = s.anchors.as<double>(), *anorm = anchors + (size_t)A * dp;
    TRY(gather_anchor_rows(c, s, rows, anchors));
    if (A < s.N && A > 2) {   // the same rows again, in chain order (every row its own anchor: no buckets to order)
        std::vector<double> host((size_t)A * dp);
        DBGSOM_HIP_CHECK(hipMemcpyAsync(host.data(), anchors, (size_t)A * dp * 8, hipMemcpyDeviceToHost, c->stream));
        DBGSOM_HIP_CHECK(hipStreamSynchronize(c->stream));
        chain_anchors(host, A, dp, rows);
        TRY(gather_anchor_rows(c, s, rows, anchors));
    }
    if (A == s.N) {
        hipLaunchKernelGGL(iota_i32_kernel, dim3(grid1d(s.N)), dim3(256), 0, c->stream, s.anchor_of.as<int32_t>(),
                           s.anchor_order.as<int32_t>(), s.N);
        TRY(launch_status("iota_i32_kernel"));
    } else {
        TRY(launch_row_sqnorms(anchors, DBGSOM_F64, A, dp, dp, anorm, c->stream));
        TRY(c->filt_ws.reserve_zeroed(dbgsom_bmu_filtered_workspace_bytes(s.N, dp, A), c->stream));
        FilteredCall call = filtered_call(c, s, anchors, A, anorm);
        call.seed_stride = DBGSOM_SEED_FULL; call.sweep_planes = 1;
        call.seeds_out = s.anchor_of.as<int32_t>(); call.order_out = s.anchor_order.as<int32_t>();
        call.ws = c->filt_ws.p; call.ws_bytes = c->filt_ws.cap;
        TRY(launch_bmu_filtered(call));
    }
    // the run table of the bucket order: what the candidate lists need of the samples, once per load (the stored
    // rows: the values the search reads, at the storage's width)
    TRY(s.anchor_runs.reserve(anchor_runs_bytes(s.N, (int)A)));
    TRY(launch_anchor_runs(s.X, s.dtype, s.N, dp, dp, s.xx.as<double>(), anchors, (int)A, s.anchor_of.as<int32_t>(),
                           s.anchor_order.as<int32_t>(), s.anchor_runs.p, s.anchor_runs.cap, c->stream));
    s.n_anchors = A;
    s.anchor_state = 1;
    ++c->anchor_builds;
    c->anchor.anchors_built();
    return DBGSOM_OK;
}

bool filter_shape_ok(const Samples &s, int64_t M) { return SearchPolicy::shape_ok(M, s.N, s.dp); }

bool filter_applies(const dbgsom_ctx *c, int64_t M) {
    if (c->xs.csr) return false;   // (no candidate pruning for CSR residents)
    return c->policy.filter_allowed() && filter_shape_ok(c->xs, M);
}

// the previous epoch's winners seed the search of the resident samples
bool hint_applies(const dbgsom_ctx *c, int64_t M) { return c->search.hint_applies(c->policy.takes_hint(), M); }

// prototypes: make W (host, or the resident ones) the consumed matrix Wb[cur]; norms into ww
int stage_weights(dbgsom_ctx *c, const double *W_host, int64_t M, int64_t d, int64_t dp) {
    DBGSOM_REQUIRE(M >= 1 && M <= 0x7fffff00, "bad prototype count");
    if (W_host) {
        TRY(c->Wb[c->cur].reserve((size_t)M * dp * 8));
        TRY(upload_padded(c, c->Wb[c->cur].p, W_host, M, d, dp, 8));
        c->search.weights_replaced(c->cur);
        c->M = M;
        ++c->w_up_calls; c->w_up_bytes += M * d * 8;
    } else if (c->M != M) {
        set_error("no resident prototypes of %lld rows (resident: %lld); pass W_host or call dbgsom_ctx_set_weights",
                  (long long)M, (long long)c->M);
        return DBGSOM_ESTATE;
    }
    TRY(c->ww.reserve((size_t)M * 8));
    return launch_row_sqnorms(c->Wb[c->cur].p, DBGSOM_F64, M, dp, dp, c->ww.as<double>(), c->stream);
}

// k = 1 search through the int8 filter, in the form the policy plans; seeds = previous winners when `prev_idx`
int run_filtered(dbgsom_ctx *c, Samples &s, DevBuf &ws, const double *W, int64_t M, int round_f32,
                 const int64_t *prev_idx, const int32_t *order, int64_t *idx, double *dist, bool may_probe = false) {
    TRY(ensure_planes(c, s));
    TRY(ws.reserve_zeroed(dbgsom_bmu_filtered_workspace_bytes(s.N, s.dp, M), c->stream));
    const ResidentSearchState &st = c->search;   // (the bound: the last epoch's distances under Wb[st.distW_buf])
    const bool bound_usable = st.bound_usable(dist == c->dist.as<double>(), c->Wb[st.distW_buf].p != nullptr);
    const SearchPolicy::Plan plan = c->policy.plan(M, s.N, s.dp, prev_idx != nullptr, may_probe, bound_usable);
    FilteredCall call = filtered_call(c, s, W, M, c->ww.as<double>());
    if (plan.hint_bound) {
        ++c->hint_bound_searches;
        TRY(c->shiftb.reserve((size_t)M * 8));
        const int64_t rows = st.distW_M < M ? st.distW_M : M;
        hipLaunchKernelGGL(row_shift_kernel, dim3((unsigned)M), dim3(64), 0, c->stream, W,
                           c->Wb[st.distW_buf].as<double>(), s.dp, s.dp, rows, M, c->shiftb.as<double>());
        TRY(launch_status("row_shift_kernel"));
        call.hint_dist = c->dist.as<double>();
        call.hint_shift = c->shiftb.as<double>();
    }
    call.prev_idx = prev_idx; call.order = order; call.seed_stride = plan.seed_stride; call.sweep_planes = plan.sweep_planes;
    // seeds from the anchor buckets instead of the pre-pass, and the lean form behind them: AnchorControl decides
    if (c->anchor.wants_anchors(plan, prev_idx != nullptr, &s == &c->xs, c->anchor_seeds != 0, s.anchor_state, M)) {
        TRY(ensure_anchors(c, s));   // (may grow `ws` for its own call: call.ws is taken below)
        ++c->anchor_searches;
        call.anchors = s.anchors.as<double>(); call.n_anchors = (int)s.n_anchors;
        call.anchor_of = s.anchor_of.as<int32_t>(); call.order = s.anchor_order.as<int32_t>();
        call.anchor_runs = s.anchor_runs.p;
        if (c->anchor.anchor_seeded(plan, M, may_probe, s.anchor_generation)) {
            call.seed_stride |= DBGSOM_ANCHOR_LISTS_ONLY;
            ++c->lean_searches;
        }
    }
    call.round_f32 = round_f32; call.idx = idx; call.dist = dist; call.ws = ws.p; call.ws_bytes = ws.cap;
    call.refine_rows = plan.refine_rows;
    c->last_refined = plan.refine;
    if (s.dtype == DBGSOM_BF16) { call.X_store = s.X; call.store_dtype = DBGSOM_BF16; call.ld_store = s.dp; }
    call.guard_mean = plan.guard_mean;
    const int rc_f = launch_bmu_filtered(call);
    c->last_filter_M = M; c->last_filter_N = s.N; c->last_filter_d = s.dp; c->last_filter_ws = ws.p;
    if (rc_f == DBGSOM_LISTS_LONG) {
        c->policy.on_guarded();
        c->last_refined = false;
        return launch_bmu(s.Xb, s.bdtype, s.N, s.dp, s.dp, s.xx.as<double>(), W, M, c->ww.as<double>(), 1, round_f32, idx,
                          dist, c->stream);
    }
    TRY(rc_f);
    return DBGSOM_OK;
}

// librccl, resolved at run time (no link-time dependency: single-GPU callers never load it)
struct RcclApi {
    int (*get_unique_id)(void *id) = nullptr;                                        // ncclGetUniqueId
    int (*comm_init_rank)(void **comm, int nranks, /* ncclUniqueId by value */ ...) = nullptr;
    int (*all_reduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*reduce_scatter)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;   // (optional)
    int (*all_gather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;            // (optional)
    int (*comm_count)(void *, int *) = nullptr;                                                     // (optional)
    int (*comm_user_rank)(void *, int *) = nullptr;                                                 // (optional)
    int (*comm_destroy)(void *) = nullptr;
    const char *(*error_string)(int) = nullptr;
    bool tried = false, ok = false;
};
struct NcclUniqueId { char internal[128]; };   // (rccl.h: ncclUniqueId)
typedef int (*nccl_comm_init_rank_fn)(void **comm, int nranks, NcclUniqueId id, int rank);
RcclApi g_rccl;
nccl_comm_init_rank_fn g_rccl_init = nullptr;

int rccl_load() {
    if (g_rccl.tried) {
        if (!g_rccl.ok) { set_error("librccl could not be loaded (see the first failure)"); return DBGSOM_ESTATE; }
        return DBGSOM_OK;
    }
    g_rccl.tried = true;
    void *h = nullptr;
    // a copy already in the process (PyTorch's) shares the HIP runtime that is in use: take it.  RTLD_DEFAULT is a
    // null pointer on glibc, so "found in the process" is a flag of its own, not a non-null handle
    const bool in_process = dlsym(RTLD_DEFAULT, "ncclAllReduce") != nullptr;
    if (in_process) h = RTLD_DEFAULT;
    const char *env = getenv("DBGSOM_RCCL_LIB");
    const char *names[] = {env, "librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
    for (const char *n : names) {
        if (in_process || h) break;
        if (n && *n) h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
    }
    if (!h && !in_process) { set_error("librccl not found (set DBGSOM_RCCL_LIB): %s", dlerror()); return DBGSOM_ESTATE; }
    g_rccl.get_unique_id = (int (*)(void *))dlsym(h, "ncclGetUniqueId");
    g_rccl_init = (nccl_comm_init_rank_fn)dlsym(h, "ncclCommInitRank");
    g_rccl.all_reduce = (int (*)(const void *, void *, size_t, int, int, void *, hipStream_t))dlsym(h, "ncclAllReduce");
    g_rccl.comm_destroy = (int (*)(void *))dlsym(h, "ncclCommDestroy");
    g_rccl.reduce_scatter = (int (*)(const void *, void *, size_t, int, int, void *, hipStream_t))dlsym(h, "ncclReduceScatter");
    g_rccl.all_gather = (int (*)(const void *, void *, size_t, int, void *, hipStream_t))dlsym(h, "ncclAllGather");
    g_rccl.comm_count = (int (*)(void *, int *))dlsym(h, "ncclCommCount");
    g_rccl.comm_user_rank = (int (*)(void *, int *))dlsym(h, "ncclCommUserRank");
    g_rccl.error_string = (const char *(*)(int))dlsym(h, "ncclGetErrorString");
    g_rccl.ok = g_rccl.get_unique_id && g_rccl_init && g_rccl.all_reduce && g_rccl.comm_destroy;
    if (!g_rccl.ok) { set_error("librccl lacks ncclGetUniqueId / ncclCommInitRank / ncclAllReduce / ncclCommDestroy"); return DBGSOM_ESTATE; }
    return DBGSOM_OK;
}
const char *rccl_err(int rc) { return g_rccl.error_string ? g_rccl.error_string(rc) : "?"; }
void drop_rccl(dbgsom_ctx *c) {
    if (c->rccl_comm && c->rccl_owned && g_rccl.ok) {
        if (c->stream) (void)hipStreamSynchronize(c->stream);
        (void)g_rccl.comm_destroy(c->rccl_comm);
    }
    if (c->rccl_comm) { c->coll_rank = 0; c->coll_nranks = 1; }
    c->rccl_comm = nullptr;
    c->rccl_owned = false;
}

int run_allreduce(dbgsom_ctx *c, double *buf, int64_t count) {
    if (c->rccl_comm) {  // ncclDouble = 8, ncclSum = 0 (rccl.h), in place, on the context's stream
        const int rc = g_rccl.all_reduce(buf, buf, (size_t)count, 8, 0, c->rccl_comm, c->stream);
        if (rc != 0) {
            (void)hipStreamSynchronize(c->stream);
            set_error("ncclAllReduce failed (%d: %s)", rc, rccl_err(rc));
            return DBGSOM_ECALLBACK;
        }
        return DBGSOM_OK;
    }
    if (c->coll) {
        const int rc = c->coll(c->coll_user, DBGSOM_COLL_ALLREDUCE, buf, count, (void *)c->stream);
        if (rc != 0) {
            (void)hipStreamSynchronize(c->stream);
            set_error("collective callback failed (all-reduce, %d)", rc);
            return DBGSOM_ECALLBACK;
        }
        return DBGSOM_OK;
    }
    if (!c->allreduce) return DBGSOM_OK;
    const int rc = c->allreduce(c->allreduce_user, buf, count, (void *)c->stream);
    if (rc != 0) {
        (void)hipStreamSynchronize(c->stream);
        set_error("all-reduce callback failed (%d)", rc);
        return DBGSOM_ECALLBACK;
    }
    return DBGSOM_OK;
}

// in place over nranks blocks of `per` values: op = DBGSOM_COLL_REDUCE_SCATTER leaves the SUM of block `rank` in
// block `rank`; DBGSOM_COLL_ALLGATHER fills every block from its owner's
int run_block_collective(dbgsom_ctx *c, int op, double *buf, int64_t per) {
    if (c->rccl_comm) {
        double *mine = buf + (size_t)c->coll_rank * per;
        const int rc = op == DBGSOM_COLL_REDUCE_SCATTER
                           ? g_rccl.reduce_scatter(buf, mine, (size_t)per, 8, 0, c->rccl_comm, c->stream)
                           : g_rccl.all_gather(mine, buf, (size_t)per, 8, c->rccl_comm, c->stream);
        if (rc != 0) {
            (void)hipStreamSynchronize(c->stream);
            set_error("%s failed (%d: %s)", op == DBGSOM_COLL_REDUCE_SCATTER ? "ncclReduceScatter" : "ncclAllGather", rc, rccl_err(rc));
            return DBGSOM_ECALLBACK;
        }
        return DBGSOM_OK;
    }
    const int rc = c->coll ? c->coll(c->coll_user, op, buf, per, (void *)c->stream) : 1;
    if (rc != 0) {
        (void)hipStreamSynchronize(c->stream);
        set_error("collective callback failed (op %d, %d)", op, rc);
        return DBGSOM_ECALLBACK;
    }
    return DBGSOM_OK;
}

// does this epoch smooth column blocks?  (a function of the options, the collective and the shape alone:
// every rank decides the same)
bool shard_smoothing(const dbgsom_ctx *c, int64_t M, int64_t dp) {
    if (c->shard_smooth == 0 || (c->coll_nranks < 2 && c->shard_smooth != 1)) return false;   // (one rank: only when forced -- tests)
    const bool can = c->rccl_comm ? (g_rccl.reduce_scatter && g_rccl.all_gather) : c->coll != nullptr;
    if (!can) return false;
    // by default only where the replicated GEMM is worth two more launches and a second collective: from
    // ~8 GFLOP (the C5 map: 68.7; the C4 map, 1.6 GFLOP in 48 us, is bound by its chain of k-tiles, not by the
    // products, and would gain nothing)
    return c->shard_smooth == 1 || 2.0 * (double)M * (double)M * (double)dp >= 8e9;
}

void mark(dbgsom_ctx *c, int k) {
    if (!c->timing) return;
    if (!c->ev_created) { for (auto &e : c->ev) (void)hipEventCreate(&e); c->ev_created = true; }
    (void)hipEventRecord(c->ev[k], c->stream);
}

// the three arrays of host CSR rows into s.indptr / s.indices / s.data, behind whatever runs on the context's stream
int upload_csr_arrays(dbgsom_ctx *c, Samples &s, const int64_t *indptr_host, const int32_t *indices_host,
                      const void *data_host, int x_dtype, int64_t N, int64_t nnz) {
    const size_t es = dtype_size(x_dtype);
    TRY(s.indptr.reserve((size_t)(N + 1) * 8));
    TRY(s.indices.reserve((size_t)(nnz > 0 ? nnz : 1) * 4));
    TRY(s.data.reserve((size_t)(nnz > 0 ? nnz : 1) * es));
    DBGSOM_HIP_CHECK(hipMemcpyAsync(s.indptr.p, indptr_host, (size_t)(N + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (nnz > 0) {
        DBGSOM_HIP_CHECK(hipMemcpyAsync(s.indices.p, indices_host, (size_t)nnz * 4, hipMemcpyHostToDevice, c->stream));
        DBGSOM_HIP_CHECK(hipMemcpyAsync(s.data.p, data_host, (size_t)nnz * es, hipMemcpyHostToDevice, c->stream));
    }
    return DBGSOM_OK;
}

// CSR samples: upload the three arrays (checked on the host first) and take the norms; below
// `densify_below` features the rows are expanded on the device into the ordinary padded form instead and `s`
// is a dense sample set like any other (the CSR arrays are then only staged)
int place_host_csr(dbgsom_ctx *c, Samples &s, const int64_t *indptr_host, const int32_t *indices_host,
                   const void *data_host, int x_dtype, int64_t N, int64_t d, int64_t nnz, int64_t densify_below) {
    DBGSOM_REQUIRE(x_dtype == DBGSOM_F32 || x_dtype == DBGSOM_F64, "CSR data must be DBGSOM_F32 or DBGSOM_F64 (no bfloat16 storage)");
    DBGSOM_REQUIRE(indptr_host && N >= 1 && d >= 1 && nnz >= 0 && N < 0x7fffffff && d <= 0x7fffffff, "bad samples");
    DBGSOM_REQUIRE(nnz == 0 || (indices_host && data_host), "null pointer");
    TRY(dbgsom_csr_check(indptr_host, indices_host, N, d, nnz));
    const size_t es = dtype_size(x_dtype);
    const int64_t dp = pad16(d);
    s.N = N; s.d = d; s.dp = dp; s.dtype = x_dtype; s.nnz = nnz; s.csr = false;
    s.X = s.Xb = nullptr;
    TRY(upload_csr_arrays(c, s, indptr_host, indices_host, data_host, x_dtype, N, nnz));
    if (d < densify_below) {
        TRY(s.own.reserve((size_t)N * dp * es));
        TRY(launch_csr_densify(s.view(), x_dtype, N, d, dp, s.own.p, c->stream));
        s.X = s.own.p;
        TRY(finish_samples(c, s, false));
        TRY(sync(c));
        s.indptr.release(); s.indices.release(); s.data.release();
        s.nnz = 0;
        return DBGSOM_OK;
    }
    s.csr = true;
    s.bdtype = x_dtype;
    s.own.release(); s.x32.release(); s.planes.release();
    s.drop_planes();
    TRY(s.xx.reserve((size_t)N * 8));
    return launch_csr_row_sqnorms(s.view(), x_dtype, N, s.xx.as<double>(), c->stream);
}

// the CSR search of `s` under the M x dp prototypes W (device) with norms ww: Wt is rebuilt from W first
int csr_search(dbgsom_ctx *c, Samples &s, const double *W, const double *ww, DevBuf &wt, int64_t M, int k, int round_f32,
               int64_t *idx, double *dist) {
    const int64_t ldwt = csr_wt_ld(M);
    TRY(wt.reserve((size_t)s.dp * ldwt * 8));
    TRY(launch_transpose_weights(W, M, s.dp, s.dp, wt.as<double>(), ldwt, c->stream));
    return launch_bmu_csr(s.view(), s.dtype, s.N, s.xx.as<double>(), wt.as<double>(), ldwt, M, ww, k, round_f32, idx,
                          dist, c->stream);
}
int csr_search(dbgsom_ctx *c, Samples &s, const double *W, int64_t M, int k, int round_f32, int64_t *idx, double *dist) {
    return csr_search(c, s, W, c->ww.as<double>(), c->wt, M, k, round_f32, idx, dist);
}

// BMU (k = 1) of the resident samples under Wb[cur] into idx[icur ^ 1] / dist, by policy
int epoch_bmu(dbgsom_ctx *c, int64_t M, int round_f32) {
    Samples &s = c->xs;
    TRY(c->idx[0].reserve((size_t)s.N * 8));
    TRY(c->idx[1].reserve((size_t)s.N * 8));
    TRY(c->dist.reserve((size_t)s.N * 8));
    int64_t *out = c->idx[c->icur ^ 1].as<int64_t>();
    const double *W = c->Wb[c->cur].as<double>();
    c->policy.begin_epoch();
    if (s.csr) {
        c->last_filtered = false;
        TRY(csr_search(c, s, W, M, 1, round_f32, out, c->dist.as<double>()));
        c->icur ^= 1;
        c->search.foreign_search_done();
        return DBGSOM_OK;
    }
    if (filter_applies(c, M)) {
        const bool hint = hint_applies(c, M);
        c->last_filtered = true;
        TRY(run_filtered(c, s, c->filt_ws, W, M, round_f32, hint ? c->idx[c->icur].as<int64_t>() : nullptr,
                         hint ? c->acc_ws.as<int32_t>() : nullptr, out, c->dist.as<double>(), true));
    } else {
        c->last_filtered = false;
        c->policy.on_exact_epoch();
        TRY(launch_bmu(s.Xb, s.bdtype, s.N, s.dp, s.dp, s.xx.as<double>(), W, M, c->ww.as<double>(), 1, round_f32,
                       out, c->dist.as<double>(), c->stream));
    }
    c->icur ^= 1;
    c->search.dense_search_done(c->cur, M);
    return DBGSOM_OK;
}

// workspace of the accumulate step: the weighted form's rows are one scalar wider
size_t acc_ws_bytes(dbgsom_ctx *c, int64_t M) {
    return c->has_weights ? accumulate_weighted_workspace_bytes(c->xs.N, c->xs.dp, M)
                          : accumulate_workspace_bytes(c->xs.N, c->xs.dp, M);
}

// sums = [S | K | a | E | status] of the resident samples for winners idx / distances dist and the
// sample weights kw (kw == nullptr: the sample kernel with `gamma`, computed inside the sums kernel)
int accumulate_and_reduce(dbgsom_ctx *c, const int64_t *idx, const double *kw, double gamma, const double *dist,
                          int64_t M) {
    Samples &s = c->xs;
    DBGSOM_REQUIRE(M <= DBGSOM_MAX_PROTOTYPES, "M exceeds DBGSOM_MAX_PROTOTYPES");
    const int64_t count = M * (s.dp + 3);
    TRY(c->sums.reserve((size_t)(count + 1) * 8));
    TRY(c->acc_ws.reserve(acc_ws_bytes(c, M)));
    TRY(c->scal.reserve(256));
    int32_t *status = reinterpret_cast<int32_t *>(c->scal.as<char>() + 64);
    c->part_valid = false;
    const double *sw = c->has_weights ? c->sw.as<double>() : nullptr;
    if (s.csr) {
        TRY(launch_accumulate_csr(s.view(), s.dtype, s.N, s.dp, idx, kw, gamma, sw, dist, M, c->sums.as<double>(), status,
                                  kw == nullptr, c->acc_ws.p, c->acc_ws.cap, c->stream));
        if (kw) {
            hipLaunchKernelGGL(status_to_f64_kernel, dim3(1), dim3(1), 0, c->stream, status, c->sums.as<double>() + count);
            TRY(launch_status("status_to_f64_kernel"));
        }
    } else if (kw) {
        if (sw)
            TRY(launch_accumulate_weighted(s.X, s.dtype, s.N, s.dp, s.dp, idx, kw, sw, dist, M, c->sums.as<double>(), status,
                                           c->acc_ws.p, c->acc_ws.cap, c->stream));
        else
            TRY(launch_accumulate(s.X, s.dtype, s.N, s.dp, s.dp, idx, kw, dist, M, c->sums.as<double>(), status,
                                  c->acc_ws.p, c->acc_ws.cap, c->stream));
        hipLaunchKernelGGL(status_to_f64_kernel, dim3(1), dim3(1), 0, c->stream, status, c->sums.as<double>() + count);
        TRY(launch_status("status_to_f64_kernel"));
    } else {
        if (sw)
            TRY(launch_accumulate_epoch_weighted(s.X, s.dtype, s.N, s.dp, s.dp, idx, gamma, sw, dist, M, c->sums.as<double>(),
                                                 status, c->acc_ws.p, c->acc_ws.cap, c->stream));
        else
            TRY(launch_accumulate_epoch(s.X, s.dtype, s.N, s.dp, s.dp, idx, gamma, dist, M, c->sums.as<double>(), status,
                                        c->acc_ws.p, c->acc_ws.cap, c->stream));
    }
    c->sumsM = M;
    c->sums_sharded = false;
    if (shard_smoothing(c, M, s.dp)) {
        // column blocks of S -> reduce-scatter: this rank's block holds the sums of all ranks for the columns it
        // smooths.  The small vectors [K | a | E | status] behind S go through an ordinary all-reduce where they lie:
        // growth and convergence are decided from them on every rank, so they must be the same bits everywhere (a
        // reduce-scatter sums each block along its own chain of ranks)
        const int G = c->coll_nranks;
        const int64_t blk = smooth_block_elems(M, s.dp, G);
        TRY(c->shard_send.reserve((size_t)G * blk * 8));
        double *send = c->shard_send.as<double>();
        TRY(launch_pack_blocks(c->sums.as<double>(), M, s.dp, G, send, c->stream));
        TRY(run_allreduce(c, c->sums.as<double>() + (size_t)M * s.dp, 3 * M + 1));
        TRY(run_block_collective(c, DBGSOM_COLL_REDUCE_SCATTER, send, blk));
        c->sums_sharded = true;
        c->sumsM = 0;   // (the S part of `sums` is this rank's share, not the reduced sums: nothing to read back)
        return DBGSOM_OK;
    }
    return run_allreduce(c, c->sums.as<double>(), count + 1);
}

// Workspace of the smoothing step.  CSR residents: carved out of the accumulate workspace behind its bucket order
// when that is large enough -- its slab rows are dead once the sums are finalized, and both steps run one after
// the other on the context's stream -- so that a wide map does not hold a second M x dp buffer for it.
int smooth_ws(dbgsom_ctx *c, int64_t M, int64_t dp, void **ws, size_t *ws_bytes) {
    const size_t need = smooth_workspace_bytes(M, dp);
    const size_t head = align_up((size_t)c->xs.N * 4);
    if (c->xs.csr && c->acc_ws.cap >= head + need) {
        *ws = c->acc_ws.as<char>() + head;
        *ws_bytes = c->acc_ws.cap - head;
        return DBGSOM_OK;
    }
    TRY(c->sm_ws.reserve(need));
    *ws = c->sm_ws.p;
    *ws_bytes = c->sm_ws.cap;
    return DBGSOM_OK;
}

// smoothing of the reduced sums: Wb[cur] -> Wb[cur ^ 1]; queues the small results D2H and waits
int smooth_and_fetch(dbgsom_ctx *c, int64_t M, double sigma, int layout, int flags, double *W_new_host,
                     double *change_total_host, double *errors_host, double *activations_host,
                     const int64_t *idx_dev, int64_t *idx_host, double *dist_host) {
    Samples &s = c->xs;
    const int64_t dp = s.dp, d = s.d;
    if (c->topoM != M) {
        set_error("topology holds %lld neurons, prototypes %lld (call dbgsom_ctx_set_topology after growth)",
                  (long long)c->topoM, (long long)M);
        return DBGSOM_ESTATE;
    }
    const int nxt = c->cur ^ 1;
    TRY(c->Wb[nxt].reserve((size_t)M * dp * 8));
    void *sm_ws = nullptr;
    size_t sm_ws_bytes = 0;
    TRY(smooth_ws(c, M, dp, &sm_ws, &sm_ws_bytes));
    double *sums = c->sums.as<double>();
    if (c->sums_sharded) {
        const int G = c->coll_nranks, r = c->coll_rank;
        const int64_t cb = smooth_block_cols(dp, G), blk = smooth_block_elems(M, dp, G);
        const double *mine = c->shard_send.as<double>() + (size_t)r * blk;
        TRY(c->shard_gather.reserve((size_t)G * M * cb * 8));
        double *gather = c->shard_gather.as<double>();
        TRY(launch_smooth_block(mine, sums + (size_t)M * dp, sums + (size_t)M * dp + M, M, cb, dp, c->hop.as<float>(), sigma,
                                layout, gather + (size_t)r * M * cb, sm_ws, sm_ws_bytes, c->stream));
        TRY(run_block_collective(c, DBGSOM_COLL_ALLGATHER, gather, M * cb));
        TRY(launch_rowchange_blocks(gather, M, dp, cb, c->Wb[c->cur].as<double>(), c->Wb[nxt].as<double>(), nullptr, sm_ws,
                                    c->stream));
        c->sums_sharded = false;
        ++c->shard_epochs;
    } else {
        TRY(launch_smooth(sums, M, dp, c->hop.as<float>(), sigma, layout, c->Wb[c->cur].as<double>(),
                          c->Wb[nxt].as<double>(), nullptr, sm_ws, sm_ws_bytes, c->stream, true));
    }
    mark(c, 3);
    // the epoch's small results: one kernel writes them into mapped page-locked memory, one stream
    // synchronisation
    TRY(c->tail.reserve((size_t)(2 * M + 6) * 8));
    double *tail = c->tail.as<double>();
    const unsigned long long *list_sum =
        c->last_filtered ? dbgsom_filter_count_sum_ptr(c->filt_ws.p, s.N, dp, M) : nullptr;
    hipLaunchKernelGGL(pack_results_kernel, dim3((unsigned)((2 * M + 255) / 256 < 64 ? (2 * M + 255) / 256 : 64)), dim3(256), 0,
                       c->stream, sums + (size_t)M * dp + M, M, smooth_rowchg(sm_ws, M, dp), sums + (size_t)M * (dp + 3), list_sum,
                       reinterpret_cast<double *>(c->tail.dev));
    TRY(launch_status("pack_results_kernel"));
    if (W_new_host) {
        TRY(download_unpadded(c, W_new_host, c->Wb[nxt].p, M, d, dp, 8));
        ++c->w_down_calls; c->w_down_bytes += M * d * 8;
    }
    if (idx_host) DBGSOM_HIP_CHECK(hipMemcpyAsync(idx_host, idx_dev, (size_t)s.N * 8, hipMemcpyDeviceToHost, c->stream));
    if (dist_host) DBGSOM_HIP_CHECK(hipMemcpyAsync(dist_host, c->dist.p, (size_t)s.N * 8, hipMemcpyDeviceToHost, c->stream));
    TRY(sync(c));
    c->ev_valid = c->timing != 0;
    if (c->timing && c->last_filtered) {
        c->filter_ms_valid = filter_stage_ms(c->faux, c->filter_ms) == DBGSOM_OK;
    } else {
        c->filter_ms_valid = false;
    }
    memcpy(activations_host, tail, (size_t)M * 8);
    memcpy(errors_host, tail + M, (size_t)M * 8);
    change_total_host[0] = tail[2 * M];
    c->otherM = M;
    if (!(flags & DBGSOM_EPOCH_FROZEN)) c->cur = nxt;  // W' becomes the resident matrix, W the "previous" one
    if (tail[2 * M + 1] != 0.0) { set_error("winner index out of range"); return DBGSOM_ERANGE; }
    return DBGSOM_OK;
}

int loaded(const dbgsom_ctx *c, const char *fn) {
    if (c->xs.dtype < 0) { set_error("%s: no samples loaded", fn); return DBGSOM_ESTATE; }
    return DBGSOM_OK;
}

// the ordinary calls never compute on rows with missing entries: a NaN would run through every distance and sum
int complete_rows(const dbgsom_ctx *c, const char *fn) {
    if (c->incomplete) {
        set_error("%s: the resident rows have missing entries (option \"incomplete\"): use dbgsom_ctx_bmu_masked / "
                  "dbgsom_ctx_epoch_masked", fn);
        return DBGSOM_EINVAL;
    }
    return DBGSOM_OK;
}

// what the masked calls need: rows marked incomplete (dense float32 / float64 by construction), no weights, one rank
int masked_ready(const dbgsom_ctx *c, const char *fn) {
    TRY(loaded(c, fn));
    const char *why = nullptr;
    if (c->xs.csr || c->xs.dtype == DBGSOM_BF16) why = "CSR and bfloat16 residents cannot have missing entries";
    else if (!c->incomplete) why = "the resident rows are not marked incomplete (option \"incomplete\")";
    else if (c->has_weights) why = "sample weights are attached";
    else if (c->coll_nranks > 1 || c->allreduce) why = "more than one rank";
    if (why) { set_error("%s: %s", fn, why); return DBGSOM_EINVAL; }
    return DBGSOM_OK;
}

// the k nearest prototypes of every resident row over its observed entries: W_host (M x d) -> mf_w, mf_idx, mf_dist
int resident_bmu_masked(dbgsom_ctx *c, const double *W_host, int64_t M, int k) {
    Samples &s = c->xs;
    TRY(masked_check_shape(s.dtype, s.N, s.d, s.dp, M, k));
    TRY(c->mf_w.reserve((size_t)M * s.d * 8));
    TRY(c->mf_wt.reserve(masked_weights_bytes(s.d, M)));
    TRY(c->mf_idx.reserve((size_t)s.N * k * 8));
    TRY(c->mf_dist.reserve((size_t)s.N * k * 8));
    DBGSOM_HIP_CHECK(hipMemcpyAsync(c->mf_w.p, W_host, (size_t)M * s.d * 8, hipMemcpyHostToDevice, c->stream));
    TRY(launch_masked_weights(c->mf_w.as<double>(), M, s.d, s.d, c->mf_wt.p, c->stream));
    const bool f32 = s.dtype == DBGSOM_F32;
    return launch_bmu_masked_prepared(f32 ? c->mf_x64.as<double>() : (const double *)s.X, s.N, s.d, f32 ? s.d : s.dp,
                                      c->mf_nobs.as<int32_t>(), c->mf_wt.as<double>(), M, k, c->mf_idx.as<int64_t>(),
                                      c->mf_dist.as<double>(), c->stream);
}

enum Metric { METRIC_MANHATTAN, METRIC_COSINE };

// what the Manhattan and cosine calls on the resident rows need: dense float32 / float64 rows, complete, no weights,
// one rank
int metric_ready(const dbgsom_ctx *c, const char *fn, Metric metric) {
    TRY(loaded(c, fn));
    const char *name = metric == METRIC_MANHATTAN ? "Manhattan" : "cosine";
    if (c->xs.csr) { set_error("%s: CSR residents have no %s search", fn, name); return DBGSOM_EINVAL; }
    if (c->xs.dtype == DBGSOM_BF16) { set_error("%s: bfloat16 storage has no %s search", fn, name); return DBGSOM_EINVAL; }
    const char *why = nullptr;
    if (c->incomplete) why = "the resident rows have missing entries (option \"incomplete\")";
    else if (c->has_weights) why = "sample weights are attached";
    else if (c->coll_nranks > 1 || c->allreduce) why = "more than one rank";
    if (why) { set_error("%s: %s", fn, why); return DBGSOM_EINVAL; }
    return DBGSOM_OK;
}

// the k nearest prototypes of every resident row under sum |x - w|: W (device, M rows ldw apart) -> idx / dist (N x k)
int resident_bmu_manhattan(dbgsom_ctx *c, const double *W, int64_t ldw, int64_t M, int k, int64_t *idx, double *dist) {
    Samples &s = c->xs;
    TRY(masked_check_shape(s.dtype, s.N, s.d, s.dp, M, k));
    TRY(c->l1_ws.reserve(bmu_manhattan_workspace_bytes(s.dtype, s.N, s.d, M)));
    TRY(launch_manhattan_weights(W, M, s.d, ldw, c->l1_ws.p, c->stream));
    return launch_bmu_manhattan_rows(s.X, s.dtype, s.N, s.d, s.dp, M, k, idx, dist, c->l1_ws.p, c->l1_ws.cap, c->stream);
}

// the k nearest prototypes of every resident row under 1 - cos: W (device, M rows of dp values) -> idx / dist (N x k).
// u = inv(|x|^2) of the resident rows is made from their resident norms on the first call after a load and kept;
// the prototypes' norms and v are made per call.
int resident_bmu_cosine(dbgsom_ctx *c, const double *W, int64_t M, int k, int64_t *idx, double *dist) {
    Samples &s = c->xs;
    if (!c->cos_u_ready) {
        TRY(c->cos_u.reserve((size_t)s.N * 8));
        TRY(launch_inv_norms(s.xx.as<double>(), s.N, c->cos_u.as<double>(), c->stream));
        c->cos_u_ready = true;
    }
    TRY(c->cos_v.reserve((size_t)M * 16));   // [squared norms | their inverses]
    double *pp = c->cos_v.as<double>(), *v = pp + M;
    TRY(launch_row_sqnorms(W, DBGSOM_F64, M, s.dp, s.dp, pp, c->stream));
    TRY(launch_inv_norms(pp, M, v, c->stream));
    return launch_bmu_cosine(s.Xb, s.bdtype, s.N, s.dp, s.dp, c->cos_u.as<double>(), W, M, v, k, idx, dist, c->stream);
}

// BMU of the resident samples for the reductions around the path: k = 1 by policy, k = 2 all-pairs.
// Results in qidx / qdist (N x k); the training hint (idx[icur], bucket order) is left alone.
int resident_bmu(dbgsom_ctx *c, const double *W_host, int64_t M, int k, int round_f32) {
    Samples &s = c->xs;
    TRY(stage_weights(c, W_host, M, s.d, s.dp));
    TRY(c->qidx.reserve((size_t)s.N * k * 8));
    TRY(c->qdist.reserve((size_t)s.N * k * 8));
    const double *W = c->Wb[c->cur].as<double>();
    if (s.csr) {
        c->last_k2_filtered = false;
        return csr_search(c, s, W, M, k, round_f32, c->qidx.as<int64_t>(), c->qdist.as<double>());
    }
    if (k == 1 && filter_applies(c, M)) {
        const bool hint = hint_applies(c, M);
        return run_filtered(c, s, c->filt_ws, W, M, round_f32, hint ? c->idx[c->icur].as<int64_t>() : nullptr,
                            hint ? c->acc_ws.as<int32_t>() : nullptr, c->qidx.as<int64_t>(), c->qdist.as<double>());
    }
    // k = 2 (topographic error, BaseSom.py:945): through the pruning form of the filtered search when the
    // training epochs have shown that it works on this data (SearchPolicy::k2_prunes); otherwise all pairs
    if (k == 2 && filter_applies(c, M) && c->policy.k2_prunes(M)) {
        const bool hint = hint_applies(c, M);
        TRY(ensure_planes(c, s));
        TRY(c->filt_ws.reserve_zeroed(dbgsom_bmu_filtered_workspace_bytes(s.N, s.dp, M), c->stream));
        FilteredCall call = filtered_call(c, s, W, M, c->ww.as<double>());
        call.prev_idx = hint ? c->idx[c->icur].as<int64_t>() : nullptr;
        call.order = hint ? c->acc_ws.as<int32_t>() : nullptr;
        call.seed_stride = c->policy.k2_seed_stride(hint);
        call.sweep_planes = 1; call.round_f32 = round_f32; call.k = 2;
        call.idx = c->qidx.as<int64_t>(); call.dist = c->qdist.as<double>();
        call.ws = c->filt_ws.p; call.ws_bytes = c->filt_ws.cap;
        c->last_k2_filtered = true;
        return launch_bmu_filtered(call);
    }
    c->last_k2_filtered = false;
    return launch_bmu(s.Xb, s.bdtype, s.N, s.dp, s.dp, s.xx.as<double>(), W, M, c->ww.as<double>(), k, round_f32,
                      c->qidx.as<int64_t>(), c->qdist.as<double>(), c->stream);
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------------------------------
// life cycle, options
// ------------------------------------------------------------------------------------------
int dbgsom_ctx_create(int device, dbgsom_ctx **out) {
    DBGSOM_REQUIRE(out, "null pointer");
    *out = nullptr;
    int n = 0;
    DBGSOM_HIP_CHECK(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) {
        set_error("dbgsom_ctx_create: device %d not available (%d visible)", device, n);
        return DBGSOM_EINVAL;
    }
    DBGSOM_HIP_CHECK(hipSetDevice(device));
    dbgsom_ctx *c = new (std::nothrow) dbgsom_ctx();
    if (!c) { set_error("out of host memory"); return DBGSOM_ENOMEM; }
    c->device = device;
    // (highest priority: the side streams of the filtered search -- a few long chains off the critical
    //  path -- must not starve the short dependent kernels of this one)
    int prio_low = 0, prio_high = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_low, &prio_high);
    hipError_t err = hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, prio_high);
    if (err != hipSuccess) { (void)hipGetLastError(); err = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking); }
    if (err != hipSuccess) {
        set_error("hipStreamCreate failed: %s", hipGetErrorString(err));
        delete c;
        return DBGSOM_EHIP;
    }
    *out = c;
    return DBGSOM_OK;
}

// every DevBuf of a context, for dbgsom_ctx_destroy and the "device_bytes" option alike
#define CTX_DEVBUFS(c)                                                                                             \
    {&(c)->y, &(c)->hop, &(c)->hop_stage, &(c)->Wb[0], &(c)->Wb[1], &(c)->ww, &(c)->idx[0], &(c)->idx[1], &(c)->dist,  \
     &(c)->kw, &(c)->sums, &(c)->acc_ws, &(c)->sm_ws, &(c)->filt_ws, &(c)->scal, &(c)->qidx, &(c)->qdist, &(c)->red,  \
     &(c)->hist, &(c)->stage_dev, &(c)->part_order, &(c)->part_ws, &(c)->part_counts, &(c)->shiftb, &(c)->shard_send,    \
     &(c)->shard_gather, &(c)->sw, &(c)->wh_order, &(c)->wh_ws, &(c)->sc_ws, &(c)->sc_x, &(c)->sc_w, &(c)->sc_p, &(c)->sc_code, &(c)->sc_proba, &(c)->sc_cnt, &(c)->wt,  \
     &(c)->mk_ws, &(c)->mk_x, &(c)->mk_w, &(c)->mk_idx, &(c)->mk_dist, &(c)->mf_nobs, &(c)->mf_x64, &(c)->mf_wt, &(c)->mf_w,   \
     &(c)->mf_wn, &(c)->mf_idx, &(c)->mf_dist, &(c)->mf_kw, &(c)->mf_sums, &(c)->mf_acc_ws, &(c)->mf_sm_ws, &(c)->mf_scal, \
     &(c)->pd_out, &(c)->kn_ws, &(c)->kn_idx, &(c)->kn_dist, &(c)->de_h, &(c)->ce_g, &(c)->ce_ws, &(c)->ex_state, &(c)->rc_state, &(c)->l1_ws, &(c)->cos_u, &(c)->cos_v,   \
     &(c)->ty, &(c)->us_ws, &(c)->us_in, &(c)->us_out, &(c)->us_dev}

int dbgsom_ctx_destroy(dbgsom_ctx *c) {
    if (!c) return DBGSOM_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    drop_rccl(c);
    c->faux.destroy();
    c->xs.release(); c->xq.release();
    DevBuf *bufs[] = CTX_DEVBUFS(c);
    for (DevBuf *b : bufs) b->release();
    c->tail.release(); c->counts.release();
    if (c->ev_created) for (auto &e : c->ev) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return DBGSOM_OK;
}

int dbgsom_ctx_set_option(dbgsom_ctx *c, const char *name, int64_t v) {
    CTX_CHECK(c);
    DBGSOM_REQUIRE(name, "null option name");
    if (!strcmp(name, "algorithm")) {
        DBGSOM_REQUIRE(v >= DBGSOM_ALG_AUTO && v <= DBGSOM_ALG_FILTERED_HINT, "algorithm must be a DBGSOM_ALG_* value");
        c->policy.algorithm = (int)v;
    } else if (!strcmp(name, "sweep_planes")) {
        DBGSOM_REQUIRE(v >= 0 && v <= 4, "sweep_planes must be 0 .. 4 (4 = no sweep: triangle pruning)");
        c->policy.sweep_planes = (int)v;
    } else if (!strcmp(name, "seed_stride")) {
        DBGSOM_REQUIRE(v >= 0 && v <= 64, "seed_stride outside [0, 64]");
        c->policy.seed_stride = (int)v;
    } else if (!strcmp(name, "timing")) {
        c->timing = v != 0;
        c->ev_valid = false;
        c->faux.timer.enabled = c->timing != 0;
        c->faux.timer.valid = false;
    } else if (!strcmp(name, "shard_smooth")) {
        DBGSOM_REQUIRE(v >= 0 && v <= 2, "shard_smooth must be 0 (never), 1 (whenever the collective can) or 2 (large maps)");
        c->shard_smooth = (int)v;
    } else if (!strcmp(name, "refine")) {
        DBGSOM_REQUIRE(v >= 0 && v <= 2, "refine must be 0 (off), 1 (on) or 2 (by measurement)");
        c->policy.set_refine((int)v);
    } else if (!strcmp(name, "filter_min_query_rows")) {
        DBGSOM_REQUIRE(v >= 0, "filter_min_query_rows must be >= 0");
        c->filter_min_query_rows = v;
    } else if (!strcmp(name, "sc_chunk_rows")) {
        DBGSOM_REQUIRE(v >= 1 && v <= ((int64_t)1 << 22), "sc_chunk_rows must be in [1, 2^22]");
        c->sc_chunk_rows = v;
    } else if (!strcmp(name, "masked_chunk_rows")) {
        DBGSOM_REQUIRE(v >= 1 && v <= ((int64_t)1 << 22), "masked_chunk_rows must be in [1, 2^22]");
        c->masked_chunk_rows = v;
    } else if (!strcmp(name, "distances_chunk_rows")) {
        DBGSOM_REQUIRE(v >= 0 && v <= ((int64_t)1 << 22), "distances_chunk_rows must be in [0, 2^22] (0 = by the result's size)");
        c->distances_chunk_rows = v;
    } else if (!strcmp(name, "kneighbors_slab_rows")) {
        DBGSOM_REQUIRE(v >= 0 && v <= ((int64_t)1 << 22), "kneighbors_slab_rows must be in [0, 2^22] (0 = by the slab's size)");
        c->kneighbors_slab_rows = v;
    } else if (!strcmp(name, "sc_cap")) {
        DBGSOM_REQUIRE(v >= 0 && v <= 64, "sc_cap must be in [0, 64] (0 = the library's cap)");
        c->sc_cap = v;
    } else if (!strcmp(name, "max_mean_candidates")) {
        DBGSOM_REQUIRE(v >= 1, "max_mean_candidates must be >= 1");
        c->policy.max_mean_candidates = v;
    } else if (!strcmp(name, "csr_densify_below")) {
        DBGSOM_REQUIRE(v >= 0, "csr_densify_below must be >= 0 (0 = CSR input always stays CSR)");
        c->csr_densify_below = v;
    } else if (!strcmp(name, "anchor_seeds")) {
        DBGSOM_REQUIRE(v == 0 || v == 1, "anchor_seeds must be 0 or 1");
        c->anchor_seeds = (int)v;
    } else if (!strcmp(name, "incomplete")) {
        // 1: NaN in the resident rows marks a missing entry (set after the load; the next load clears it)
        DBGSOM_REQUIRE(v == 0 || v == 1, "incomplete must be 0 or 1");
        c->incomplete = false;
        if (v == 0) { c->mf_nobs.release(); c->mf_x64.release(); return DBGSOM_OK; }
        TRY(loaded(c, __func__));
        Samples &s = c->xs;
        DBGSOM_REQUIRE(!s.csr && (s.dtype == DBGSOM_F32 || s.dtype == DBGSOM_F64),
                       "only dense float32 / float64 residents can be marked incomplete");
        DBGSOM_REQUIRE(!c->has_weights && c->coll_nranks == 1 && !c->allreduce,
                       "incomplete rows take neither sample weights nor more than one rank");
        TRY(c->mf_nobs.reserve((size_t)s.N * 4));
        if (s.dtype == DBGSOM_F32) TRY(c->mf_x64.reserve((size_t)s.N * s.d * 8));
        TRY(launch_masked_prepare(s.X, s.dtype, s.N, s.d, s.dp, c->mf_nobs.as<int32_t>(), c->mf_x64.as<double>(), c->stream));
        TRY(sync(c));
        c->incomplete = true;
    } else {
        set_error("dbgsom_ctx_set_option: unknown option '%s'", name);
        return DBGSOM_EINVAL;
    }
    return DBGSOM_OK;
}

int dbgsom_ctx_get_option(dbgsom_ctx *c, const char *name, int64_t *v) {
    CTX_CHECK(c);
    DBGSOM_REQUIRE(name && v, "null pointer");
    if (!strcmp(name, "algorithm")) *v = c->policy.algorithm;
    else if (!strcmp(name, "sweep_planes")) *v = c->policy.sweep_planes;
    else if (!strcmp(name, "seed_stride")) *v = c->policy.seed_stride;
    else if (!strcmp(name, "timing")) *v = c->timing;
    else if (!strcmp(name, "refine")) *v = c->policy.refine;
    else if (!strcmp(name, "refined")) *v = c->last_refined ? 1 : 0;
    else if (!strcmp(name, "shard_smooth")) *v = c->shard_smooth;
    else if (!strcmp(name, "shard_epochs")) *v = c->shard_epochs;
    else if (!strcmp(name, "guarded_calls")) *v = c->policy.guarded_calls;
    else if (!strcmp(name, "collective_rank")) *v = c->coll_rank;
    else if (!strcmp(name, "collective_ranks")) *v = c->coll_nranks;
    else if (!strcmp(name, "k2_filtered")) *v = c->last_k2_filtered ? 1 : 0;
    else if (!strcmp(name, "filter_min_query_rows")) *v = c->filter_min_query_rows;
    else if (!strcmp(name, "max_mean_candidates")) *v = c->policy.max_mean_candidates;
    else if (!strcmp(name, "sc_chunk_rows")) *v = c->sc_chunk_rows;
    else if (!strcmp(name, "sc_cap")) *v = c->sc_cap;
    else if (!strcmp(name, "masked_chunk_rows")) *v = c->masked_chunk_rows;
    else if (!strcmp(name, "distances_chunk_rows")) *v = c->distances_chunk_rows;
    else if (!strcmp(name, "kneighbors_slab_rows")) *v = c->kneighbors_slab_rows;
    else if (!strcmp(name, "csr_densify_below")) *v = c->csr_densify_below;
    else if (!strcmp(name, "resident_csr")) *v = (c->xs.dtype >= 0 && c->xs.csr) ? 1 : 0;
    else if (!strcmp(name, "resident_nnz")) *v = (c->xs.dtype >= 0 && c->xs.csr) ? c->xs.nnz : 0;
    else if (!strcmp(name, "n_samples")) *v = c->xs.dtype < 0 ? 0 : c->xs.N;
    else if (!strcmp(name, "features")) *v = c->xs.dtype < 0 ? 0 : c->xs.d;
    else if (!strcmp(name, "padded_features")) *v = c->xs.dtype < 0 ? 0 : c->xs.dp;
    else if (!strcmp(name, "storage")) *v = c->xs.dtype;
    else if (!strcmp(name, "prototypes")) *v = c->M;
    else if (!strcmp(name, "planes_cached")) *v = c->xs.planes_ready ? 1 : 0;
    else if (!strcmp(name, "anchor_seeds")) *v = c->anchor_seeds;
    else if (!strcmp(name, "incomplete")) *v = c->incomplete ? 1 : 0;
    else if (!strcmp(name, "anchor_builds")) *v = c->anchor_builds;
    else if (!strcmp(name, "anchor_searches")) *v = c->anchor_searches;
    else if (!strcmp(name, "lean_searches")) *v = c->lean_searches;
    else if (!strcmp(name, "hint_bound_searches")) *v = c->hint_bound_searches;
    else if (!strcmp(name, "anchor_state")) *v = c->xs.dtype < 0 ? 0 : c->xs.anchor_state;
    else if (!strcmp(name, "planes_used")) *v = c->policy.planes_used;
    else if (!strcmp(name, "planes_next")) *v = c->policy.planes_for_call();
    else if (!strcmp(name, "hint_valid")) *v = c->search.hint_valid ? 1 : 0;
    else if (!strcmp(name, "filter_backoff")) *v = c->policy.filter_backoff;
    else if (!strcmp(name, "plane_hold")) *v = c->policy.plane_hold;
    else if (!strcmp(name, "seed_mode")) *v = c->policy.seed_mode;
    else if (!strcmp(name, "prune_retry")) *v = c->policy.prune_retry ? 1 : 0;
    else if (!strcmp(name, "w_upload_calls")) *v = c->w_up_calls;
    else if (!strcmp(name, "w_upload_bytes")) *v = c->w_up_bytes;
    else if (!strcmp(name, "w_download_calls")) *v = c->w_down_calls;
    else if (!strcmp(name, "w_download_bytes")) *v = c->w_down_bytes;
    else if (!strcmp(name, "w_row_writes")) *v = c->w_row_writes;
    else if (!strcmp(name, "w_row_reads")) *v = c->w_row_reads;
    else if (!strcmp(name, "x_upload_bytes")) *v = c->x_up_bytes;
    else if (!strcmp(name, "x_upload_calls")) *v = c->x_up_calls;
    else if (!strcmp(name, "x_download_bytes")) *v = c->x_down_bytes;
    else if (!strcmp(name, "device_bytes")) {
        size_t tot = 0;
        for (const Samples *q : {&c->xs, &c->xq})
            tot += q->own.cap + q->x32.cap + q->xx.cap + q->planes.cap + q->indptr.cap + q->indices.cap + q->data.cap +
                   q->anchors.cap + q->anchor_of.cap + q->anchor_order.cap + q->anchor_runs.cap;
        DevBuf *bufs[] = CTX_DEVBUFS(c);
        for (DevBuf *b : bufs) tot += b->cap;
        *v = (int64_t)tot;
    } else {
        set_error("dbgsom_ctx_get_option: unknown option '%s'", name);
        return DBGSOM_EINVAL;
    }
    return DBGSOM_OK;
}

int dbgsom_ctx_stream(dbgsom_ctx *c, void **stream) {
    CTX_CHECK(c);
    DBGSOM_REQUIRE(stream, "null pointer");
    *stream = (void *)c->stream;
    return DBGSOM_OK;
}

// ------------------------------------------------------------------------------------------
// residency
// ------------------------------------------------------------------------------------------
// the allocation policy of every buffer of the context (DevBuf::tight): tight for CSR residents
static void set_tight(dbgsom_ctx *c, bool tight) {
    DevBuf *bufs[] = CTX_DEVBUFS(c);
    for (DevBuf *b : bufs) b->tight = tight;
    for (Samples *q : {&c->xs, &c->xq})
        for (DevBuf *b : {&q->own, &q->x32, &q->xx, &q->planes, &q->indptr, &q->indices, &q->data, &q->anchors, &q->anchor_of,
                          &q->anchor_order, &q->anchor_runs})
            b->tight = tight;
}

static void reset_training_state(dbgsom_ctx *c) {
    c->search.reset();
    c->part_valid = false;
    c->has_labels = false;
    c->has_weights = false;
    c->has_targets = false;
    c->incomplete = false;
    c->cos_u_ready = false;   // (u belongs to the rows that were resident)
    c->policy.reset();
    c->anchor.reset();
    c->last_filtered = false;
    c->sumsM = 0;
    // the resident prototypes were laid out for the old samples' padded row length: gone with them
    c->M = c->otherM = 0;
}

int dbgsom_ctx_load(dbgsom_ctx *c, const void *X_host, int x_dtype, int64_t N, int64_t d, int storage) {
    CTX_CHECK(c);
    reset_training_state(c);
    set_tight(c, false);
    c->xs.dtype = -1;
    c->xs.indptr.release(); c->xs.indices.release(); c->xs.data.release();
    const int rc = place_host_samples(c, c->xs, X_host, x_dtype, N, d, storage);
    if (rc != DBGSOM_OK) { (void)hipStreamSynchronize(c->stream); c->xs.dtype = -1; return rc; }
    return sync(c);
}

int dbgsom_ctx_load_csr(dbgsom_ctx *c, const int64_t *indptr_host, const int32_t *indices_host, const void *data_host,
                        int x_dtype, int64_t N, int64_t d, int64_t nnz) {
    CTX_CHECK(c);
    reset_training_state(c);
    c->xs.dtype = -1;
    set_tight(c, d >= c->csr_densify_below);
    int rc = place_host_csr(c, c->xs, indptr_host, indices_host, data_host, x_dtype, N, d, nnz, c->csr_densify_below);
    if (rc == DBGSOM_OK) rc = sync(c);
    if (rc != DBGSOM_OK) { (void)hipStreamSynchronize(c->stream); c->xs.dtype = -1; c->xs.csr = false; }
    else c->x_up((size_t)nnz * (4 + dtype_size(x_dtype)) + (size_t)(N + 1) * 8);
    return rc;
}

int dbgsom_ctx_load_device(dbgsom_ctx *c, const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx) {
    CTX_CHECK(c);
    DBGSOM_REQUIRE(valid_dtype(x_dtype), "x_dtype must be DBGSOM_F32/F64/BF16");
    DBGSOM_REQUIRE(X_dev && N >= 1 && d >= 1 && ldx >= d && N < 0x7fffffff, "bad samples");
    reset_training_state(c);
    set_tight(c, false);
    Samples &s = c->xs;
    const int rc = place_device_samples(c, s, X_dev, x_dtype, N, d, ldx);
    if (rc != DBGSOM_OK) { (void)hipStreamSynchronize(c->stream); s.dtype = -1; return rc; }
    return sync(c);
}

int dbgsom_ctx_read_samples(dbgsom_ctx *c, const int64_t *rows_host, int64_t n, double *out_host) {
    CTX_CHECK(c);
    TRY(loaded(c, __func__));
    DBGSOM_REQUIRE(n >= 0 && (n == 0 || (rows_host && out_host)), "bad arguments");
    if (n == 0) return DBGSOM_OK;
    Samples &s = c->xs;
    for (int64_t r = 0; r < n; ++r) DBGSOM_REQUIRE(rows_host[r] >= 0 && rows_host[r] < s.N, "row index out of range");
    TRY(c->stage_dev.reserve((size_t)n * 8 + (size_t)n * s.d * 8 + 256));
    int64_t *ids = c->stage_dev.as<int64_t>();
    double *rows = reinterpret_cast<double *>(c->stage_dev.as<char>() + align_up((size_t)n * 8));
    DBGSOM_HIP_CHECK(hipMemcpyAsync(ids, rows_host, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    if (s.csr) {   // densified rows
        TRY(launch_csr_rows_to_f64(s.view(), s.dtype, ids, n, s.d, rows, c->stream));
        DBGSOM_HIP_CHECK(hipMemcpyAsync(out_host, rows, (size_t)n * s.d * 8, hipMemcpyDeviceToHost, c->stream));
        return sync(c);
    }
    if (s.dtype == DBGSOM_F32)
        hipLaunchKernelGGL(rows_to_f64_kernel<float>, dim3((unsigned)n), dim3(256), 0, c->stream, (const float *)s.X, s.dp, ids, n, s.d, rows);
    else if (s.dtype == DBGSOM_F64)
        hipLaunchKernelGGL(rows_to_f64_kernel<double>, dim3((unsigned)n), dim3(256), 0, c->stream, (const double *)s.X, s.dp, ids, n, s.d, rows);
    else
        hipLaunchKernelGGL(rows_to_f64_kernel<bf16_t>, dim3((unsigned)n), dim3(256), 0, c->stream, (const bf16_t *)s.X, s.dp, ids, n, s.d, rows);
    TRY(launch_status("rows_to_f64_kernel"));
    DBGSOM_HIP_CHECK(hipMemcpyAsync(out_host, rows, (size_t)n * s.d * 8, hipMemcpyDeviceToHost, c->stream));
    return sync(c);
}

int dbgsom_ctx_set_labels(dbgsom_ctx *c, const int32_t *y_host, int64_t N) {
    CTX_CHECK(c);
    TRY(loaded(c, __func__));
    if (!y_host) { c->has_labels = false; return DBGSOM_OK; }
    DBGSOM_REQUIRE(N == c->xs.N, "one label per resident sample");
    TRY(c->y.reserve((size_t)N * 4));
    DBGSOM_HIP_CHECK(hipMemcpyAsync(c->y.p, y_host, (size_t)N * 4, hipMemcpyHostToDevice, c->stream));
    c->has_labels = true;
    return sync(c);
}

int dbgsom_ctx_set_sample_weight(dbgsom_ctx *c, const double *w_host, int64_t N) {
    CTX_CHECK(c);
    TRY(loaded(c, __func__));
    // (the bucket order of the last accumulate step keeps its meaning either way: a permutation of all rows)
    if (!w_host) { c->has_weights = false; return DBGSOM_OK; }
    DBGSOM_REQUIRE(N == c->xs.N, "one weight per resident sample");
    for (int64_t i = 0; i < N; ++i)
        if (!(w_host[i] >= 0.0) || w_host[i] == INFINITY) {
            set_error("dbgsom_ctx_set_sample_weight: weight %lld is negative or not finite", (long long)i);
            return DBGSOM_EINVAL;
        }
    TRY(c->sw.reserve((size_t)N * 8));
    DBGSOM_HIP_CHECK(hipMemcpyAsync(c->sw.p, w_host, (size_t)N * 8, hipMemcpyHostToDevice, c->stream));
    c->has_weights = true;
    c->sumsM = 0;
    return sync(c);
}

int dbgsom_ctx_weight_total(dbgsom_ctx *c, double *out_host) {
    CTX_CHECK(c);
    TRY(loaded(c, __func__));
    DBGSOM_REQUIRE(out_host, "null pointer");
    if (!c->has_weights) { *out_host = (double)c->xs.N; return DBGSOM_OK; }
    TRY(c->red.reserve(256 + dbgsom_sum_workspace_bytes()));
    double *r = c->red.as<double>();
    TRY(dbgsom_weighted_sum_f64(nullptr, c->sw.as<double>(), c->xs.N, r, c->red.as<char>() + 256, c->red.cap - 256, c->stream));
    DBGSOM_HIP_CHECK(hipMemcpyAsync(out_host, r, 8, hipMemcpyDeviceToHost, c->stream));
    return sync(c);
}

int dbgsom_ctx_set_topology(dbgsom_ctx *c, const double *hop_host, int64_t M) {
    CTX_CHECK(c);
    DBGSOM_REQUIRE(hop_host && M >= 1 && M <= DBGSOM_MAX_PROTOTYPES, "bad topology");
    const int64_t n = M * M;
    TRY(c->hop_stage.reserve((size_t)n * 8));
    TRY(c->hop.reserve((size_t)n * 4));
    DBGSOM_HIP_CHECK(hipMemcpyAsync(c->hop_stage.p, hop_host, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(f64_to_f32_kernel, dim3(grid1d(n)), dim3(256), 0, c->stream, c->hop_stage.as<double>(),
                       c->hop.as<float>(), n);
    TRY(launch_status("f64_to_f32_kernel"));
    TRY(sync(c));
    c->topoM = M;
    return DBGSOM_OK;
}

int dbgsom_ctx_set_collectives(dbgsom_ctx *c, dbgsom_collective_fn fn, void *user, int rank, int nranks) {
    CTX_CHECK(c);
    DBGSOM_REQUIRE(!fn || (nranks >= 1 && rank >= 0 && rank < nranks), "rank outside [0, nranks)");
    drop_rccl(c);
    c->allreduce = nullptr;
    c->allreduce_user = nullptr;
    c->coll = fn;
    c->coll_user = user;
    c->coll_rank = fn ? rank : 0;
    c->coll_nranks = fn ? nranks : 1;
    return DBGSOM_OK;
}

int dbgsom_ctx_set_allreduce(dbgsom_ctx *c, dbgsom_allreduce_fn fn, void *user) {
    CTX_CHECK(c);
    drop_rccl(c);
    c->allreduce = fn;
    c->allreduce_user = user;
    c->coll = nullptr; c->coll_user = nullptr; c->coll_rank = 0; c->coll_nranks = 1;
    return DBGSOM_OK;
}

int dbgsom_rccl_unique_id(char *id128) {
    DBGSOM_REQUIRE(id128, "null pointer");
    TRY(rccl_load());
    NcclUniqueId id;
    const int rc = g_rccl.get_unique_id(&id);
    if (rc != 0) { set_error("ncclGetUniqueId failed (%d: %s)", rc, rccl_err(rc)); return DBGSOM_ECALLBACK; }
    memcpy(id128, id.internal, 128);
    return DBGSOM_OK;
}

int dbgsom_rccl_comm_init(const char *id128, int nranks, int rank, void **comm_out) {
    DBGSOM_REQUIRE(id128 && comm_out && nranks >= 1 && rank >= 0 && rank < nranks, "bad communicator arguments");
    TRY(rccl_load());
    NcclUniqueId id;
    memcpy(id.internal, id128, 128);
    void *comm = nullptr;
    const int rc = g_rccl_init(&comm, nranks, id, rank);
    if (rc != 0 || !comm) { set_error("ncclCommInitRank failed (%d: %s)", rc, rccl_err(rc)); return DBGSOM_ECALLBACK; }
    *comm_out = comm;
    return DBGSOM_OK;
}

int dbgsom_rccl_comm_destroy(void *comm) {
    if (!comm) return DBGSOM_OK;
    TRY(rccl_load());
    const int rc = g_rccl.comm_destroy(comm);
    if (rc != 0) { set_error("ncclCommDestroy failed (%d: %s)", rc, rccl_err(rc)); return DBGSOM_ECALLBACK; }
    return DBGSOM_OK;
}

int dbgsom_ctx_allreduce_host(dbgsom_ctx *c, double *vals_host, int64_t n) {
    CTX_CHECK(c);
    DBGSOM_REQUIRE(vals_host && n >= 1, "bad arguments");
    if (!c->rccl_comm && !c->allreduce && !c->coll) return DBGSOM_OK;
    TRY(c->red.reserve((size_t)n * 8));
    DBGSOM_HIP_CHECK(hipMemcpyAsync(c->red.p, vals_host, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    TRY(run_allreduce(c, c->red.as<double>(), n));
    DBGSOM_HIP_CHECK(hipMemcpyAsync(vals_host, c->red.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    return sync(c);
}

int dbgsom_ctx_set_rccl(dbgsom_ctx *c, void *nccl_comm) {
    CTX_CHECK(c);
    if (nccl_comm) TRY(rccl_load());
    drop_rccl(c);
    c->rccl_comm = nccl_comm;
    c->rccl_owned = false;
    c->coll_rank = 0; c->coll_nranks = 1;
    if (nccl_comm) {
        c->allreduce = nullptr; c->allreduce_user = nullptr;
        c->coll = nullptr; c->coll_user = nullptr;
        // rank and size of the communicator: what the sharded smoothing needs (absent symbols: it stays off)
        int n = 1, r = 0;
        if (g_rccl.comm_count && g_rccl.comm_user_rank && g_rccl.comm_count(nccl_comm, &n) == 0 &&
            g_rccl.comm_user_rank(nccl_comm, &r) == 0 && n >= 1 && r >= 0 && r < n) {
            c->coll_nranks = n;
            c->coll_rank = r;
        }
    }
    return DBGSOM_OK;
}

// ------------------------------------------------------------------------------------------
// prototypes
// ------------------------------------------------------------------------------------------
int dbgsom_ctx_set_weights(dbgsom_ctx *c, const double *W_host, int64_t M) {
    CTX_CHECK(c);
    TRY(loaded(c, __func__));
    DBGSOM_REQUIRE(W_host && M >= 1, "bad prototypes");
    TRY(c->Wb[c->cur].reserve((size_t)M * c->xs.dp * 8));
    TRY(upload_padded(c, c->Wb[c->cur].p, W_host, M, c->xs.d, c->xs.dp, 8));
    c->search.weights_replaced(c->cur);
    c->M = M;
    ++c->w_up_calls; c->w_up_bytes += M * c->xs.d * 8;
    return sync(c);
}

int dbgsom_ctx_get_weights(dbgsom_ctx *c, int which, double *W_host, int64_t M) {
    CTX_CHECK(c);
    TRY(loaded(c, __func__));
    DBGSOM_REQUIRE(W_host && (which == 0 || which == 1), "bad arguments");
    const int b = which ? c->cur ^ 1 : c->cur;
    const int64_t have = which ? c->otherM : c->M;
    if (have != M || M < 1) {
        set_error("dbgsom_ctx_get_weights: buffer %d holds %lld rows, %lld asked for", which, (long long)have, (long long)M);
        return DBGSOM_ESTATE;
    }
    TRY(download_unpadded(c, W_host, c->Wb[b].p, M, c->xs.d, c->xs.dp, 8));
    ++c->w_down_calls; c->w_down_bytes += M * c->xs.d * 8;
    return sync(c);
}

int dbgsom_ctx_read_weight_rows(dbgsom_ctx *c, int which, const int64_t *rows_host, int64_t n, double *out_host) {
    CTX_CHECK(c);
    TRY(loaded(c, __func__));
    DBGSOM_REQUIRE((which == 0 || which == 1) && n >= 0 && (n == 0 || (rows_host && out_host)), "bad arguments");
    const int b = which ? c->cur ^ 1 : c->cur;
    const int64_t have = which ? c->otherM : c->M;
    const int64_t d = c->xs.d, dp = c->xs.dp;
    c->w_row_reads += n;
    for (int64_t r = 0; r < n; ++r) {
        DBGSOM_REQUIRE(rows_host[r] >= 0 && rows_host[r] < have, "row index out of range");
        DBGSOM_HIP_CHECK(hipMemcpyAsync(out_host + r * d, c->Wb[b].as<double>() + rows_host[r] * dp, (size_t)d * 8,
                                        hipMemcpyDeviceToHost, c->stream));
    }
    return sync(c);
}

int dbgsom_ctx_write_weight_rows(dbgsom_ctx *c, int64_t row0, int64_t n, const double *rows_host) {
    CTX_CHECK(c);
    TRY(loaded(c, __func__));
    DBGSOM_REQUIRE(n >= 0 && row0 >= 0 && row0 <= c->M && (n == 0 || rows_host), "rows must lie in [0, M] (row0 == M appends)");
    if (n == 0) return DBGSOM_OK;
    const int64_t d = c->xs.d, dp = c->xs.dp;
    const int64_t newM = row0 + n > c->M ? row0 + n : c->M;
    TRY(c->Wb[c->cur].reserve_keep((size_t)newM * dp * 8, (size_t)c->M * dp * 8, c->stream));
    double *dst = c->Wb[c->cur].as<double>() + row0 * dp;
    TRY(upload_padded(c, dst, rows_host, n, d, dp, 8));
    c->search.weights_replaced(c->cur);
    c->M = newM;
    c->w_row_writes += n;
    return sync(c);
}

// ------------------------------------------------------------------------------------------
// BMU
// ------------------------------------------------------------------------------------------
int dbgsom_ctx_bmu(dbgsom_ctx *c, const double *W_host, int64_t M, int k, int round_f32, int64_t *idx_host,
                   double *dist_host) {
    CTX_CHECK(c);
    TRY(loaded(c, __func__));
    TRY(complete_rows(c, __func__));
    DBGSOM_REQUIRE(idx_host && (k == 1 || k == 2), "bad arguments");
    DBGSOM_REQUIRE(M >= k, "need k <= M");
    TRY(resident_bmu(c, W_host, M, k, round_f32));
    DBGSOM_HIP_CHECK(hipMemcpyAsync(idx_host, c->qidx.p, (size_t)c->xs.N * k * 8, hipMemcpyDeviceToHost, c->stream));
    c->x_down((size_t)c->xs.N * k * 8);
    if (dist_host) {
        DBGSOM_HIP_CHECK(hipMemcpyAsync(dist_host, c->qdist.p, (size_t)c->xs.N * k * 8, hipMemcpyDeviceToHost, c->stream));
        c->x_down((size_t)c->xs.N * k * 8);
    }
    return sync(c);
}

// the query search on samples that are not resident: dense rows from the host or from HBM (q), or CSR arrays from
// the host (indptr_host != nullptr, q.p = their data).  Rows from the host: idx_out / dist_out are host arrays,
// filled by a copy behind the search.  Rows in HBM: they are device arrays and the search writes them itself.
static int bmu_query_impl(dbgsom_ctx *c, const QueryRows &q, const int64_t *indptr_host, const int32_t *indices_host,
                          int64_t nnz, int x_dtype, int64_t Nq, int64_t d, const double *W_host, int64_t M, int k,
                          int round_f32, int64_t *idx_out, double *dist_out) {
    Samples &s = c->xq;
    DevBuf Wq, wwq, iq, dq, fws, wtq;  // query-sized scratch; independent of the training state
    int rc = DBGSOM_OK;
    const int64_t dp = pad16(d);
    do {
        if (indptr_host) {
            rc = place_host_csr(c, s, indptr_host, indices_host, q.p, x_dtype, Nq, d, nnz, c->csr_densify_below);
            if (rc == DBGSOM_OK) c->x_up((size_t)nnz * (4 + dtype_size(x_dtype)) + (size_t)(Nq + 1) * 8);
        } else {
            rc = place_query_rows(c, s, q, x_dtype, Nq, d);
        }
        if (rc) break;
        if ((rc = Wq.reserve((size_t)M * dp * 8))) break;
        if ((rc = wwq.reserve((size_t)M * 8))) break;
        int64_t *idx_dev = idx_out;
        double *dist_dev = dist_out;
        if (!q.on_device) {
            if ((rc = iq.reserve((size_t)Nq * k * 8))) break;
            if ((rc = dq.reserve((size_t)Nq * k * 8))) break;
            idx_dev = iq.as<int64_t>();
            dist_dev = dq.as<double>();
        }
        if ((rc = upload_padded(c, Wq.p, W_host, M, d, dp, 8))) break;
        if ((rc = launch_row_sqnorms(Wq.p, DBGSOM_F64, M, dp, dp, wwq.as<double>(), c->stream))) break;
        // large k = 1 queries go through the filter (the digit planes of a one-off X cost a pass over it)
        const bool filt = !s.csr && k == 1 && c->policy.algorithm != DBGSOM_ALG_EXACT && Nq >= c->filter_min_query_rows &&
                          filter_shape_ok(s, M);
        if (s.csr) {
            rc = csr_search(c, s, Wq.as<double>(), wwq.as<double>(), wtq, M, k, round_f32, idx_dev, dist_dev);
        } else if (filt) {
            if ((rc = ensure_planes(c, s))) break;
            if ((rc = fws.reserve_zeroed(dbgsom_bmu_filtered_workspace_bytes(Nq, dp, M), c->stream))) break;
            int stride = 0, planes = 1;
            c->policy.query_args(M, &stride, &planes);
            rc = dbgsom_bmu_filtered(s.Xb, s.bdtype, Nq, dp, dp, s.xx.as<double>(), s.planes.p, Wq.as<double>(), M,
                                     wwq.as<double>(), nullptr, nullptr, stride, planes, round_f32,
                                     idx_dev, dist_dev, fws.p, fws.cap, c->stream);
        } else {
            rc = launch_bmu(s.Xb, s.bdtype, Nq, dp, dp, s.xx.as<double>(), Wq.as<double>(), M, wwq.as<double>(), k,
                            round_f32, idx_dev, dist_dev, c->stream);
        }
        if (rc) break;
        hipError_t e = hipSuccess;
        if (!q.on_device) {
            e = hipMemcpyAsync(idx_out, iq.p, (size_t)Nq * k * 8, hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(dist_out, dq.p, (size_t)Nq * k * 8, hipMemcpyDeviceToHost, c->stream);
            c->x_down((size_t)Nq * k * 16);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) { set_error("D2H copy failed: %s", hipGetErrorString(e)); rc = DBGSOM_EHIP; }
    } while (0);
    if (rc != DBGSOM_OK) (void)hipStreamSynchronize(c->stream);
    Wq.release(); wwq.release(); iq.release(); dq.release(); fws.release(); wtq.release();
    const int64_t held = s.csr ? s.nnz * (4 + (int64_t)dtype_size(x_dtype)) + Nq * 16 : Nq * dp * (int64_t)dtype_size(x_dtype);
    drop_query_rows(s, q, held);
    return rc;
}

int dbgsom_ctx_bmu_query(dbgsom_ctx *c, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d, const double *W_host,
                         int64_t M, int k, int round_f32, int64_t *idx_host, double *dist_host) {
    CTX_CHECK(c);
    DBGSOM_REQUIRE(valid_dtype(x_dtype), "x_dtype must be DBGSOM_F32/F64/BF16");
    DBGSOM_REQUIRE(Xq_host && W_host && idx_host && dist_host && Nq >= 0 && d >= 1 && M >= 1 && (k == 1 || k == 2) && M >= k,
                   "bad arguments");
    if (Nq == 0) return DBGSOM_OK;
    return bmu_query_impl(c, QueryRows{Xq_host, false, d}, nullptr, nullptr, 0, x_dtype, Nq, d, W_host, M, k, round_f32,
                          idx_host, dist_host);
}

int dbgsom_ctx_bmu_query_device(dbgsom_ctx *c, const void *Xq_dev, int x_dtype, int64_t Nq, int64_t d, int64_t ldx,
                                const double *W_host, int64_t M, int k, int round_f32, int64_t *idx_dev, double *dist_dev) {
    CTX_CHECK(c);
    DBGSOM_REQUIRE(valid_dtype(x_dtype), "x_dtype must be DBGSOM_F32/F64/BF16");
    DBGSOM_REQUIRE(Xq_dev && W_host && idx_dev && dist_dev && Nq >= 0 && d >= 1 && ldx >= d && M >= 1 &&
                       (k == 1 || k == 2) && M >= k,
                   "bad arguments");
    if (Nq == 0) return DBGSOM_OK;
    return bmu_query_impl(c, QueryRows{Xq_dev, true, ldx}, nullptr, nullptr, 0, x_dtype, Nq, d, W_host, M, k, round_f32,
                          idx_dev, dist_dev);
}

int dbgsom_ctx_bmu_query_csr(dbgsom_ctx *c, const int64_t *indptr_host, const int32_t *indices_host, const void *data_host,
                             int x_dtype, int64_t Nq, int64_t d, int64_t nnz, const double *W_host, int64_t M, int k,
                             int round_f32, int64_t *idx_host, double *dist_host) {
    CTX_CHECK(c);
    DBGSOM_REQUIRE(x_dtype == DBGSOM_F32 || x_dtype == DBGSOM_F64, "CSR data must be DBGSOM_F32 or DBGSOM_F64");
    DBGSOM_REQUIRE(indptr_host && W_host && idx_host && dist_host && Nq >= 0 && d >= 1 && nnz >= 0 && M >= 1 &&
                   (k == 1 || k == 2) && M >= k, "bad arguments");
    if (Nq == 0) return dbgsom_csr_check(indptr_host, indices_host, 0, d, nnz);
    return bmu_query_impl(c, QueryRows{data_host, false, d}, indptr_host, indices_host, nnz, x_dtype, Nq, d, W_host, M, k,
                          round_f32, idx_host, dist_host);
}

// ------------------------------------------------------------------------------------------
// The chunked query drivers.  Every query beside the plain BMU search above -- the distance matrix and the k nearest
// prototypes under every metric, and the search itself over rows with missing entries and under metric="manhattan"
// and metric="cosine" -- is one of two loops over chunks of rows:
//   raw_rows_query     masked / Manhattan / cosine: kernels that read the rows as they are stored (any row pitch)
//   placed_rows_query  Euclidean distances, neighbours, distortion, exemplars, range counts, mixture view, combined
//                      error and the nearest resident rows: the rows go through the query placement first
// A chunk of host rows goes up, its result is staged on the device and comes down behind the kernel; rows in HBM are
// read where they are and the kernels write the caller's device arrays.  Both drivers synchronise before they return,
// on error too (W_host and the rows are pageable), and end on drop_large_query_scratch.  The exported calls further
// down are their argument checks (query_args and the three *_checked functions) and one call of a driver.
// ------------------------------------------------------------------------------------------
namespace {

enum QueryOp { Q_BMU, Q_DISTANCES, Q_KNEIGHBORS, Q_DISTORTION, Q_EXEMPLARS, Q_COMBINED, Q_RANGE_COUNTS, Q_MIXTURE,
               Q_ROW_NEIGHBORS };
enum RowsForm { ROWS_MASKED, ROWS_MANHATTAN, ROWS_COSINE };

// DBGSOM_REQUIRE under the name of the exported call `fn` (checks shared by several of them)
#define REQUIRE_FN(fn, cond, msg) \
    do { if (!(cond)) { set_error("%s: %s", fn, msg); return DBGSOM_EINVAL; } } while (0)

constexpr int64_t DISTANCES_STAGE_BYTES = (int64_t)256 << 20;

// rows per chunk: the option, or as many as keep the staged result -- and the staged rows -- of a chunk at 256 MiB
int64_t distances_chunk(const dbgsom_ctx *c, int64_t Nq, int64_t M, int64_t row_bytes) {
    int64_t rows = c->distances_chunk_rows;
    if (rows < 1) rows = std::max<int64_t>(128, std::min(DISTANCES_STAGE_BYTES / (M * 8), DISTANCES_STAGE_BYTES / row_bytes));
    return std::max<int64_t>(1, std::min(rows, Nq));
}

// shape checks of the distance matrix and of the k nearest prototypes
int query_args(const char *fn, const dbgsom_ctx *c, QueryOp op, int x_dtype, bool masked_or_csr, int64_t Nq, int64_t d,
               int64_t M, int k) {
    if (!c) { set_error("%s: null context", fn); return DBGSOM_EINVAL; }
    const bool dt_ok = masked_or_csr ? (x_dtype == DBGSOM_F32 || x_dtype == DBGSOM_F64) : valid_dtype(x_dtype);
    if (!dt_ok) {
        set_error("%s: x_dtype must be %s", fn, masked_or_csr ? "DBGSOM_F32 or DBGSOM_F64" : "DBGSOM_F32/F64/BF16");
        return DBGSOM_EINVAL;
    }
    REQUIRE_FN(fn, Nq >= 0 && Nq < 0x7fffffff && d >= 1 && d <= 0x7fffffff, "bad sample shape");
    REQUIRE_FN(fn, M >= 1 && M <= DBGSOM_MAX_PROTOTYPES, "need 1 <= M <= DBGSOM_MAX_PROTOTYPES");
    if (op == Q_DISTANCES || op == Q_DISTORTION || op == Q_MIXTURE) return DBGSOM_OK;
    if (op == Q_RANGE_COUNTS) {   // (k counts thresholds)
        REQUIRE_FN(fn, k >= 1 && k <= DBGSOM_MAX_RADII, "need 1 <= n_radii <= DBGSOM_MAX_RADII");
        return DBGSOM_OK;
    }
    if (op == Q_EXEMPLARS || op == Q_ROW_NEIGHBORS) REQUIRE_FN(fn, k >= 1, "need k >= 1");   // (k counts rows: it may exceed M, and Nq)
    else REQUIRE_FN(fn, k >= 1 && k <= M, "need 1 <= k <= M");
    REQUIRE_FN(fn, k <= DBGSOM_MAX_NEIGHBORS, "k must be <= DBGSOM_MAX_NEIGHBORS");
    return DBGSOM_OK;
}

int64_t first_row_without_entries(const void *X, int x_dtype, int64_t N, int64_t d) {
    for (int64_t i = 0; i < N; ++i) {
        int64_t c = 0;
        if (x_dtype == DBGSOM_F32) {
            const float *x = static_cast<const float *>(X) + i * d;
            while (c < d && x[c] != x[c]) ++c;
        } else {
            const double *x = static_cast<const double *>(X) + i * d;
            while (c < d && x[c] != x[c]) ++c;
        }
        if (c == d) return i;
    }
    return -1;
}

// after a query: do not sit on the scratch of a large one-off batch
void drop_large_query_scratch(dbgsom_ctx *c) {
    if (c->mk_ws.cap + c->mk_x.cap > ((size_t)256 << 20)) {
        c->mk_ws.release(); c->mk_x.release(); c->mk_idx.release(); c->mk_dist.release();
    }
    for (DevBuf *b : {&c->pd_out, &c->kn_ws, &c->de_h, &c->ce_g, &c->ce_ws, &c->ex_state, &c->rc_state})
        if (b->cap > (size_t)DISTANCES_STAGE_BYTES / 2) b->release();
}

// the end of both drivers
int finish_query(dbgsom_ctx *c, int rc) {
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (rc == DBGSOM_OK && e != hipSuccess) {
        set_error("hipStreamSynchronize failed: %s", hipGetErrorString(e));
        rc = DBGSOM_EHIP;
    }
    drop_large_query_scratch(c);
    return rc;
}

// Staged result rows down behind their kernel, counted as sample traffic: n x idx_vals indices (where there are any)
// to idx_host and n x res_vals values to res_host
static int download_rows(dbgsom_ctx *c, int64_t n, int64_t *idx_host, const int64_t *idx, int64_t idx_vals,
                         double *res_host, const double *res, int64_t res_vals) {
    hipError_t e = hipSuccess;
    if (idx_vals) e = hipMemcpyAsync(idx_host, idx, (size_t)n * idx_vals * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && res_vals)
        e = hipMemcpyAsync(res_host, res, (size_t)n * res_vals * 8, hipMemcpyDeviceToHost, c->stream);
    c->x_down((size_t)n * (idx_vals + res_vals) * 8);
    if (e != hipSuccess) { set_error("D2H copy failed: %s", hipGetErrorString(e)); return DBGSOM_EHIP; }
    return DBGSOM_OK;
}

// One raw-rows query: what it computes, on what, and the scratch that is its form's own.  What the forms do
// differently are the three switches below; a new metric is a case in each.
struct RawQuery {
    QueryOp op;
    RowsForm form;
    int x_dtype;
    int64_t d, M;
    int k;
    int64_t chunk;   // rows per chunk
    DevBuf *ws;      // masked, Manhattan: the form's workspace, the prepared prototypes in front (kn_ws for the
                     // neighbours, mk_ws otherwise); cosine: kn_ws, used for the neighbours only
    DevBuf vq, uq;   // cosine (call-local): [squared norms | their inverses] of the prototypes, of one chunk of rows
};

// reserve and size the workspace
int raw_rows_reserve(dbgsom_ctx *c, RawQuery &r) {
    const bool knn = r.op == Q_KNEIGHBORS;
    const int64_t slab = c->kneighbors_slab_rows;
    switch (r.form) {
    case ROWS_MASKED:
        return r.ws->reserve(knn ? kneighbors_masked_workspace_bytes(r.x_dtype, r.chunk, r.d, r.M, slab)
                                 : bmu_masked_workspace_bytes(r.x_dtype, r.chunk, r.d, r.M));
    case ROWS_MANHATTAN:
        return r.ws->reserve(knn ? kneighbors_manhattan_workspace_bytes(r.x_dtype, r.chunk, r.d, r.M, slab)
                                 : bmu_manhattan_workspace_bytes(r.x_dtype, r.chunk, r.d, r.M));
    case ROWS_COSINE:
        if (knn) TRY(r.ws->reserve(kneighbors_workspace_bytes(r.chunk, r.M, slab)));
        TRY(r.vq.reserve((size_t)r.M * 16));
        return r.uq.reserve((size_t)r.chunk * 16);
    }
    return DBGSOM_OK;
}

// prepare the prototypes once per call, from their copy W (M x d)
int raw_rows_prepare(dbgsom_ctx *c, RawQuery &r, const double *W) {
    switch (r.form) {
    case ROWS_MASKED: return launch_masked_weights(W, r.M, r.d, r.d, r.ws->p, c->stream);
    case ROWS_MANHATTAN: return launch_manhattan_weights(W, r.M, r.d, r.d, r.ws->p, c->stream);
    case ROWS_COSINE:
        TRY(launch_row_sqnorms(W, DBGSOM_F64, r.M, r.d, r.d, r.vq.as<double>(), c->stream));
        return launch_inv_norms(r.vq.as<double>(), r.M, r.vq.as<double>() + r.M, c->stream);
    }
    return DBGSOM_OK;
}

// launch the op on one chunk: n rows at X (ldx apart) -> idx (n x k) and res (n x k, or the matrix with rows ld_res apart)
int raw_rows_launch(dbgsom_ctx *c, RawQuery &r, const double *W, const void *X, int64_t n, int64_t ldx, int64_t *idx,
                    double *res, int64_t ld_res) {
    const int64_t slab = c->kneighbors_slab_rows;
    void *ws = r.ws->p;
    const size_t cap = r.ws->cap;
    hipStream_t s = c->stream;
    switch (r.form) {
    case ROWS_MASKED:
        if (r.op == Q_BMU) return launch_bmu_masked_rows(X, r.x_dtype, n, r.d, ldx, r.M, r.k, idx, res, ws, cap, s);
        if (r.op == Q_DISTANCES) return launch_distances_masked_rows(X, r.x_dtype, n, r.d, ldx, r.M, res, ld_res, ws, cap, s);
        return launch_kneighbors_masked_rows(X, r.x_dtype, n, r.d, ldx, r.M, r.k, slab, idx, res, ws, cap, s);
    case ROWS_MANHATTAN:
        if (r.op == Q_BMU) return launch_bmu_manhattan_rows(X, r.x_dtype, n, r.d, ldx, r.M, r.k, idx, res, ws, cap, s);
        if (r.op == Q_DISTANCES) return launch_distances_manhattan_rows(X, r.x_dtype, n, r.d, ldx, r.M, res, ld_res, ws, cap, s);
        return launch_kneighbors_manhattan_rows(X, r.x_dtype, n, r.d, ldx, r.M, r.k, slab, idx, res, ws, cap, s);
    case ROWS_COSINE: {
        // (no padded copy of the rows: the register-staged form takes any row pitch; their norms are made per chunk)
        const double *v = r.vq.as<double>() + r.M;
        double *u = r.uq.as<double>() + r.chunk;
        TRY(launch_row_sqnorms(X, r.x_dtype, n, r.d, ldx, r.uq.as<double>(), s));
        TRY(launch_inv_norms(r.uq.as<double>(), n, u, s));
        if (r.op == Q_BMU) return launch_bmu_cosine(X, r.x_dtype, n, r.d, ldx, u, W, r.M, v, r.k, idx, res, s);
        if (r.op == Q_DISTANCES) return launch_distances_cosine(X, r.x_dtype, n, r.d, ldx, u, W, r.M, v, res, ld_res, s);
        return launch_kneighbors_cosine(X, r.x_dtype, n, r.d, ldx, u, W, r.M, v, r.k, slab, idx, res, ws, cap, s);
    }
    }
    return DBGSOM_OK;
}

// One masked, Manhattan or cosine query in chunks of rows: masked_chunk_rows for the search, distances_chunk for the
// matrix and the neighbours.  Rows from the host (q.on_device false): a chunk goes up into mk_x, its result is staged
// (mk_idx / mk_dist, pd_out, kn_idx / kn_dist) and comes down behind the kernel.  Rows in HBM (Manhattan, cosine): the
// kernels read them where they are, q.ldx elements apart, and write the caller's device arrays.  idx_out / dist_out:
// Nq x k (Q_DISTANCES: dist_out is the matrix, rows ldo apart).  Masked rows: a row without an observed entry is
// refused under the name `fn`; Xfilled_host (Q_BMU, or null): every chunk is filled from its winners where it was
// staged and copied there.
int raw_rows_query(dbgsom_ctx *c, const char *fn, QueryOp op, RowsForm form, const QueryRows &q, int x_dtype, int64_t Nq,
                   int64_t d, const double *W_host, int64_t M, int k, int64_t *idx_out, double *dist_out, int64_t ldo,
                   void *Xfilled_host) {
    if (form == ROWS_MASKED) {
        const int64_t bad = first_row_without_entries(q.p, x_dtype, Nq, d);
        if (bad >= 0) { set_error("%s: row %lld has no observed entry", fn, (long long)bad); return DBGSOM_EINVAL; }
    }
    const size_t es = dtype_size(x_dtype);
    const bool knn = op == Q_KNEIGHBORS;
    RawQuery r{op, form, x_dtype, d, M, k, 0, knn ? &c->kn_ws : &c->mk_ws, DevBuf(), DevBuf()};
    r.chunk = op == Q_BMU ? std::min<int64_t>(Nq, c->masked_chunk_rows) : distances_chunk(c, Nq, M, d * 8);
    DevBuf &si = knn ? c->kn_idx : c->mk_idx, &sd = op == Q_DISTANCES ? c->pd_out : (knn ? c->kn_dist : c->mk_dist);
    const int64_t per_row = op == Q_DISTANCES ? M : k;   // values of a row's result
    int rc = DBGSOM_OK;
    do {
        if ((rc = raw_rows_reserve(c, r))) break;
        if ((rc = c->mk_w.reserve((size_t)M * d * 8))) break;
        if (!q.on_device) {
            if ((rc = c->mk_x.reserve((size_t)r.chunk * d * es))) break;
            if (op != Q_DISTANCES && (rc = si.reserve((size_t)r.chunk * k * 8))) break;
            if ((rc = sd.reserve((size_t)r.chunk * per_row * 8))) break;
        }
        hipError_t e = hipMemcpyAsync(c->mk_w.p, W_host, (size_t)M * d * 8, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) { set_error("H2D copy failed: %s", hipGetErrorString(e)); rc = DBGSOM_EHIP; break; }
        const double *W = c->mk_w.as<double>();
        if ((rc = raw_rows_prepare(c, r, W))) break;
        for (int64_t r0 = 0; r0 < Nq && rc == DBGSOM_OK; r0 += r.chunk) {
            const int64_t n = std::min(r.chunk, Nq - r0);
            const void *X = static_cast<const char *>(q.p) + (size_t)r0 * q.ldx * es;
            int64_t ldx = q.ldx, ld_res = op == Q_DISTANCES ? ldo : k;
            int64_t *idx = idx_out ? idx_out + r0 * k : nullptr;
            double *res = dist_out + r0 * ld_res;
            if (!q.on_device) {
                e = hipMemcpyAsync(c->mk_x.p, X, (size_t)n * d * es, hipMemcpyHostToDevice, c->stream);
                if (e != hipSuccess) { set_error("H2D copy failed: %s", hipGetErrorString(e)); rc = DBGSOM_EHIP; break; }
                c->x_up((size_t)n * d * es);
                X = c->mk_x.p; ldx = d;
                idx = si.as<int64_t>(); res = sd.as<double>(); ld_res = per_row;
            }
            rc = raw_rows_launch(c, r, W, X, n, ldx, idx, res, ld_res);
            if (rc || q.on_device) continue;
            rc = download_rows(c, n, idx_out ? idx_out + r0 * k : nullptr, idx, op == Q_DISTANCES ? 0 : k,
                               dist_out + r0 * per_row, res, per_row);
            if (rc == DBGSOM_OK && Xfilled_host) {
                if ((rc = launch_fill_missing(c->mk_x.p, x_dtype, n, d, d, W, M, d, idx, k, c->stream))) break;
                e = hipMemcpyAsync(static_cast<char *>(Xfilled_host) + (size_t)r0 * d * es, c->mk_x.p, (size_t)n * d * es,
                                   hipMemcpyDeviceToHost, c->stream);
                c->x_down((size_t)n * d * es);
                if (e != hipSuccess) { set_error("D2H copy failed: %s", hipGetErrorString(e)); rc = DBGSOM_EHIP; }
            }
        }
    } while (0);
    rc = finish_query(c, rc);
    r.vq.release(); r.uq.release();
    return rc;
}

// the prototypes of a Euclidean query on the device, padded, with their norms
int place_query_weights(dbgsom_ctx *c, DevBuf &Wq, DevBuf &wwq, const double *W_host, int64_t M, int64_t d, int64_t dp) {
    TRY(Wq.reserve((size_t)M * dp * 8));
    TRY(wwq.reserve((size_t)M * 8));
    TRY(upload_padded(c, Wq.p, W_host, M, d, dp, 8));
    return launch_row_sqnorms(Wq.p, DBGSOM_F64, M, dp, dp, wwq.as<double>(), c->stream);
}

// The geodesics of a map on the device (csrc/geodesics.hip): the edges go up into ce_ws behind its status word, their
// lengths are formed over Wq (rows dp apart) and G over all M sources lands in ce_g, rows M apart.  `tail` bytes are
// kept free behind the lengths.  The launches are queued; the status word is read with geodesics_status(ce_status).
struct GeoScratch {
    uint32_t *status;
    int32_t *edges;
    double *len;
    char *tail;
};

GeoScratch carve_geodesics(dbgsom_ctx *c, int64_t E) {
    char *base = static_cast<char *>(c->ce_ws.p);
    GeoScratch g;
    g.status = reinterpret_cast<uint32_t *>(base);
    g.edges = reinterpret_cast<int32_t *>(base + 256);
    g.len = reinterpret_cast<double *>(base + 256 + align_up((size_t)E * 8));
    g.tail = base + 256 + 2 * align_up((size_t)E * 8);
    return g;
}

int queue_geodesics(dbgsom_ctx *c, const double *Wq, int64_t M, int64_t d, int64_t dp, const int32_t *edges_host, int64_t E,
                    size_t tail) {
    TRY(c->ce_ws.reserve(256 + 2 * align_up((size_t)E * 8) + tail));
    TRY(c->ce_g.reserve((size_t)M * M * 8));
    const GeoScratch g = carve_geodesics(c, E);
    DBGSOM_HIP_CHECK(hipMemsetAsync(g.status, 0, 4, c->stream));
    if (E > 0) {
        DBGSOM_HIP_CHECK(hipMemcpyAsync(g.edges, edges_host, (size_t)E * 8, hipMemcpyHostToDevice, c->stream));
        c->x_up((size_t)E * 8);
        TRY(launch_edge_lengths(Wq, M, d, dp, g.edges, E, g.len, g.status, c->stream));
    }
    return launch_geodesic_rows(g.edges, g.len, E, M, nullptr, M, c->ce_g.as<double>(), M, g.status, c->stream);
}

// host CSR rows: the index arrays beside q.p, their data
struct CsrHost {
    const int64_t *indptr;
    const int32_t *indices;
    int64_t nnz;
};

// One placed-rows query: what it computes, on what, the caller's result arrays (on the host for host and CSR rows, on
// the device for rows in HBM), the operands that are its op's own, and the layout of its result.  What the ops do
// differently are the four switches below; a new query is a case in each.
struct PlacedQuery {
    QueryOp op;
    int x_dtype;
    int64_t d, M;
    int k;   // Q_KNEIGHBORS; Q_COMBINED: the 2 units; Q_EXEMPLARS: rows per prototype; Q_RANGE_COUNTS: thresholds; else 1
    int64_t *idx_out;
    double *res_out;
    int64_t ldo = 0;                       // Q_DISTANCES: rows of res_out are ldo apart (host calls: M)
    const double *H_host = nullptr;        // Q_DISTORTION: M x M
    int own_cell = 0;                      // Q_EXEMPLARS
    const double *thr_host = nullptr;      // Q_RANGE_COUNTS: k squared radii
    const int32_t *edges_host = nullptr;   // Q_COMBINED: E pairs of units
    int64_t E = 0;
    // Q_MIXTURE: the log-priors (M), c, the per-unit values Y (M x n_values, contiguous) and the third result q (Nq x
    // n_values, contiguous; host or device as the other two)
    const double *logprior_host = nullptr, *Y_host = nullptr;
    double c = 0.0, *q_out = nullptr;
    int n_values = 0;
    int n_probe = 0;                       // Q_ROW_NEIGHBORS: units probed per row (k: the rows listed per row)
    int64_t dp = 0, chunk = 0;   // set by the driver: padded features; rows per chunk (rows in HBM: all of them)
    // The layout of the result (placed_rows_layout): idx_vals indices and res_vals values per result row, and third_vals
    // more values in a third array (q_out).  Rows from the host: the indices are staged in kn_idx, the values in
    // res_stage, the third array in pd_out.  per_call: the result rows are the M prototypes' and exist after the last
    // chunk only; otherwise every row of X has one and they come down chunk by chunk.
    int64_t idx_vals = 0, res_vals = 0, third_vals = 0;
    DevBuf *res_stage = nullptr;
    bool per_call = false;
};

static void placed_rows_layout(dbgsom_ctx *c, PlacedQuery &p) {
    p.idx_vals = p.res_vals = p.k;
    p.res_stage = &c->kn_dist;
    switch (p.op) {
    case Q_DISTANCES: p.idx_vals = 0; p.res_vals = p.M; p.res_stage = &c->pd_out; break;   // the matrix alone
    case Q_COMBINED: p.res_vals = 1; break;                                                 // a pair of units, one e
    case Q_MIXTURE: p.third_vals = p.n_values; break;                                       // unit, lse and q
    case Q_EXEMPLARS: p.per_call = true; break;                                             // M x k (row, distance) pairs
    // the M x k counts live in rc_state and placed_rows_finish copies them out: nothing goes through the staging
    case Q_RANGE_COUNTS: p.per_call = true; p.idx_vals = p.res_vals = 0; break;
    default: break;   // Q_KNEIGHBORS: k and k; Q_DISTORTION (k = 1): unit and e
    }
}

// Reserve the scratch of the op (all but the staging of its result) and do what it needs once per call, in front of
// the chunks.  Wq: the placed prototypes.  What goes up here counts as sample traffic, one upload per op.
static int placed_rows_setup(dbgsom_ctx *c, const PlacedQuery &p, const double *Wq) {
    const int64_t M = p.M, slab = c->kneighbors_slab_rows;
    switch (p.op) {
    case Q_KNEIGHBORS:   // (csrc/kneighbors.hip) a chunk's squared distances live slab by slab in kn_ws
        return c->kn_ws.reserve(kneighbors_workspace_bytes(p.chunk, M, slab));
    case Q_DISTORTION:   // (csrc/distortion.hip) the neighbours' slab; H goes up into de_h
        TRY(c->de_h.reserve((size_t)M * M * 8));
        DBGSOM_HIP_CHECK(hipMemcpyAsync(c->de_h.p, p.H_host, (size_t)M * M * 8, hipMemcpyHostToDevice, c->stream));
        c->x_up((size_t)M * M * 8);
        return c->kn_ws.reserve(kneighbors_workspace_bytes(p.chunk, M, slab));
    case Q_MIXTURE: {   // (csrc/mixture.hip) the neighbours' slab; [the log-priors | Y] go up into de_h
        const size_t V = (size_t)p.n_values;
        TRY(c->de_h.reserve((size_t)M * (1 + V) * 8));
        DBGSOM_HIP_CHECK(hipMemcpyAsync(c->de_h.p, p.logprior_host, (size_t)M * 8, hipMemcpyHostToDevice, c->stream));
        if (V)
            DBGSOM_HIP_CHECK(hipMemcpyAsync(c->de_h.as<double>() + M, p.Y_host, (size_t)M * V * 8, hipMemcpyHostToDevice,
                                            c->stream));
        c->x_up((size_t)M * (1 + V) * 8);
        return c->kn_ws.reserve(kneighbors_workspace_bytes(p.chunk, M, slab));
    }
    case Q_COMBINED:   // (csrc/geodesics.hip) the geodesics of the map are queued; a chunk's n x 2 distances go behind them
        return queue_geodesics(c, Wq, M, p.d, p.dp, p.edges_host, p.E, (size_t)p.chunk * 16);
    case Q_EXEMPLARS:   // (csrc/exemplars.hip) every chunk folds into the state in ex_state: [r: M x k | row: M x k]
        TRY(c->kn_ws.reserve(exemplars_fold_workspace_bytes(p.chunk, M, p.k, slab)));
        TRY(c->ex_state.reserve((size_t)M * p.k * 16));
        return launch_topk_cols_init(c->ex_state.as<double>(), c->ex_state.as<int64_t>() + M * p.k, M, p.k, c->stream);
    case Q_RANGE_COUNTS: {   // (csrc/density.hip) rc_state: [the counts, zeroed here | the thresholds, which go up]
        const size_t counts = (size_t)M * p.k * 8;
        TRY(c->kn_ws.reserve(range_counts_workspace_bytes(p.chunk, M, slab)));
        TRY(c->rc_state.reserve(align_up(counts) + (size_t)p.k * 8));
        DBGSOM_HIP_CHECK(hipMemcpyAsync(static_cast<char *>(c->rc_state.p) + align_up(counts), p.thr_host, (size_t)p.k * 8,
                                        hipMemcpyHostToDevice, c->stream));
        DBGSOM_HIP_CHECK(hipMemsetAsync(c->rc_state.p, 0, counts, c->stream));
        c->x_up((size_t)p.k * 8);
        return DBGSOM_OK;
    }
    case Q_ROW_NEIGHBORS:   // (csrc/row_neighbors.hip) the neighbours' slab; a chunk's probe lists live in ex_state:
                            // [units: chunk x n_probe int64 | their distances: chunk x n_probe]
        TRY(c->ex_state.reserve((size_t)p.chunk * p.n_probe * 16));
        return c->kn_ws.reserve(kneighbors_workspace_bytes(p.chunk, M, slab));
    default: return DBGSOM_OK;   // Q_DISTANCES (csrc/distances.hip): no scratch
    }
}

// Launch the op on one placed chunk: the n rows in s, rows r0 .. r0 + n - 1 of the query -> idx, res and third, the
// chunk's part of a result with a row per row of X (a per_call result takes shape in the op's own scratch)
static int placed_rows_launch(dbgsom_ctx *c, const PlacedQuery &p, const Samples &s, const double *Wq, const double *wwq,
                              int64_t n, int64_t r0, int64_t *idx, double *res, double *third) {
    const int64_t M = p.M, dp = p.dp, slab = c->kneighbors_slab_rows;
    const double *xx = s.xx.as<double>();
    void *ws = c->kn_ws.p;
    const size_t cap = c->kn_ws.cap;
    hipStream_t st = c->stream;
    switch (p.op) {
    case Q_DISTANCES: return launch_distances(s.Xb, s.bdtype, n, dp, dp, xx, Wq, M, wwq, res, p.ldo, st);
    case Q_KNEIGHBORS: return launch_kneighbors(s.Xb, s.bdtype, n, dp, dp, xx, Wq, M, wwq, p.k, slab, idx, res, ws, cap, st);
    case Q_DISTORTION:   // idx / res: a row's unit and its e
        return launch_neighborhood_energy(s.Xb, s.bdtype, n, dp, dp, xx, Wq, M, wwq, c->de_h.as<double>(), M, slab, idx, res,
                                          ws, cap, st);
    case Q_MIXTURE: {   // idx / res: a row's unit and its lse; third: its q, n_values apart
        const double *a = c->de_h.as<double>();
        const int V = p.n_values;
        return launch_mixture(s.Xb, s.bdtype, n, dp, dp, xx, Wq, M, wwq, a, p.c, V ? a + M : nullptr, V, V, slab, idx, res,
                              third, V, ws, cap, st);
    }
    case Q_COMBINED: {   // the all-pairs search leaves the chunk's pairs in idx and its distances in ce_ws; the rows
                         // kernel reads both and G and writes e
        const GeoScratch g = carve_geodesics(c, p.E);
        double *d2 = reinterpret_cast<double *>(g.tail);
        TRY(launch_bmu(s.Xb, s.bdtype, n, dp, dp, xx, Wq, M, wwq, 2, 0, idx, d2, st));
        return launch_combined_error_rows(idx, d2, 2, n, c->ce_g.as<double>(), M, M, res, g.status, st);
    }
    case Q_EXEMPLARS:   // row0 = the chunk's first row
        return launch_exemplars_fold(s.Xb, s.bdtype, n, dp, dp, xx, Wq, M, wwq, p.k, p.own_cell, slab, r0,
                                     c->ex_state.as<double>(), c->ex_state.as<int64_t>() + M * p.k, ws, cap, st);
    case Q_RANGE_COUNTS: {
        const double *thr = reinterpret_cast<const double *>(static_cast<char *>(c->rc_state.p) + align_up((size_t)M * p.k * 8));
        return launch_range_counts_fold(s.Xb, s.bdtype, n, dp, dp, xx, Wq, M, wwq, thr, p.k, slab, c->rc_state.as<int64_t>(),
                                        ws, cap, st);
    }
    case Q_ROW_NEIGHBORS: {   // the chunk's nearest units, then the scan of the resident rows filed under them
        const Samples &x = c->xs;
        int64_t *units = c->ex_state.as<int64_t>();
        double *udist = reinterpret_cast<double *>(units + p.chunk * p.n_probe);
        TRY(launch_kneighbors(s.Xb, s.bdtype, n, dp, dp, xx, Wq, M, wwq, p.n_probe, slab, units, udist, ws, cap, st));
        return launch_scan_cells("dbgsom_ctx_row_neighbors_query", x.X, x.dtype, x.N, x.d, x.dp,
                                 c->part_order.as<int32_t>(), bucket_sort_seg_start(c->part_ws.p, x.N, c->partM), M, s.Xb,
                                 s.bdtype, n, dp, units, p.n_probe, p.k, idx, res, st);
    }
    default: return DBGSOM_OK;
    }
}

// After the last chunk.  idx / res: where M rows of a per_call result go (staged: the staging, which then comes down
// in one piece; else the caller's device arrays).
static int placed_rows_finish(dbgsom_ctx *c, const PlacedQuery &p, bool staged, int64_t *idx, double *res) {
    const int64_t M = p.M;
    switch (p.op) {
    case Q_COMBINED:   // what the geodesics and the rows kernels found
        return geodesics_status("dbgsom_ctx_combined_error_query", carve_geodesics(c, p.E).status, M, c->stream);
    case Q_EXEMPLARS:   // the state as the M x k result
        TRY(launch_exemplars_store(c->ex_state.as<double>(), c->ex_state.as<int64_t>() + M * p.k, M, p.k, idx, res, c->stream));
        return staged ? download_rows(c, M, p.idx_out, idx, p.k, p.res_out, res, p.k) : DBGSOM_OK;
    case Q_RANGE_COUNTS:   // the counts, from where they were folded
        if (staged) return download_rows(c, M, p.idx_out, c->rc_state.as<int64_t>(), p.k, nullptr, nullptr, 0);
        DBGSOM_HIP_CHECK(hipMemcpyAsync(p.idx_out, c->rc_state.p, (size_t)M * p.k * 8, hipMemcpyDeviceToDevice, c->stream));
        return DBGSOM_OK;
    default: return DBGSOM_OK;
    }
}

// One Euclidean query of rows that go through the query placement.  Host rows: in chunks of distances_chunk rows, each
// placed, its result rows staged and copied down behind the kernels.  Rows in HBM: placed whole, and the kernels write
// the caller's device arrays.  CSR rows (csr != nullptr): the three arrays go up whole, and chunks of rows are
// expanded into the dense rows the kernels read.  What is launched, on which scratch, is the op's (the switches
// above); where result rows go and what comes down is read off the layout.
int placed_rows_query(dbgsom_ctx *c, PlacedQuery &p, const QueryRows &q, const CsrHost *csr, int64_t Nq, const double *W_host) {
    Samples &s = c->xq;
    DevBuf Wq, wwq;
    const int x_dtype = p.x_dtype;
    const int64_t d = p.d, dp = p.dp = pad16(d);
    const size_t es = dtype_size(x_dtype);
    const bool staged = !q.on_device;
    p.chunk = staged ? distances_chunk(c, Nq, p.M, dp * (int64_t)es) : Nq;
    placed_rows_layout(c, p);
    const bool down = staged && !p.per_call;                              // result rows come down chunk by chunk
    const size_t stage_rows = !staged ? 0 : (p.per_call ? p.M : p.chunk);   // result rows that are staged at a time
    int rc = DBGSOM_OK;
    do {
        if (csr) {
            s.release();
            if ((rc = upload_csr_arrays(c, s, csr->indptr, csr->indices, q.p, x_dtype, Nq, csr->nnz))) break;
            c->x_up((size_t)csr->nnz * (4 + es) + (size_t)(Nq + 1) * 8);
            if ((rc = s.own.reserve((size_t)p.chunk * dp * es))) break;
        }
        if ((rc = place_query_weights(c, Wq, wwq, W_host, p.M, d, dp))) break;
        if ((rc = placed_rows_setup(c, p, Wq.as<double>()))) break;
        if ((rc = c->kn_idx.reserve(stage_rows * p.idx_vals * 8))) break;
        if ((rc = p.res_stage->reserve(stage_rows * p.res_vals * 8))) break;
        if ((rc = c->pd_out.reserve(stage_rows * p.third_vals * 8))) break;
        // (rows in HBM are one chunk: the caller's arrays are written from their first row)
        int64_t *idx = staged ? c->kn_idx.as<int64_t>() : p.idx_out;
        double *res = staged ? p.res_stage->as<double>() : p.res_out;
        double *third = !p.third_vals ? nullptr : (staged ? c->pd_out.as<double>() : p.q_out);
        for (int64_t r0 = 0; r0 < Nq && rc == DBGSOM_OK; r0 += p.chunk) {
            const int64_t n = std::min(p.chunk, Nq - r0);
            if (csr) {
                const CsrView rows{s.indptr.as<int64_t>() + r0, s.indices.as<int32_t>(), s.data.p};   // (indptr is absolute)
                if ((rc = launch_csr_densify(rows, x_dtype, n, d, dp, s.own.p, c->stream))) break;
                s.N = n; s.d = d; s.dp = dp; s.dtype = x_dtype; s.csr = false; s.nnz = 0;
                s.X = s.own.p;
                rc = finish_samples(c, s, false);
            } else if (q.on_device) {
                rc = place_query_rows(c, s, q, x_dtype, Nq, d);
            } else {
                rc = place_host_samples(c, s, static_cast<const char *>(q.p) + (size_t)r0 * d * es, x_dtype, n, d, x_dtype);
            }
            if (rc == DBGSOM_OK) rc = placed_rows_launch(c, p, s, Wq.as<double>(), wwq.as<double>(), n, r0, idx, res, third);
            if (rc == DBGSOM_OK && down)
                rc = download_rows(c, n, p.idx_out + r0 * p.idx_vals, idx, p.idx_vals, p.res_out + r0 * p.res_vals, res,
                                   p.res_vals);
            if (rc == DBGSOM_OK && down && p.third_vals)
                rc = download_rows(c, n, nullptr, nullptr, 0, p.q_out + r0 * p.third_vals, third, p.third_vals);
        }
        if (rc == DBGSOM_OK) rc = placed_rows_finish(c, p, staged, idx, res);
    } while (0);
    rc = finish_query(c, rc);
    Wq.release(); wwq.release();
    if (csr) s.release();
    else drop_query_rows(s, q, p.chunk * dp * (int64_t)es);
    return rc;
}

// ---- the argument checks of the exported calls, shared where a host / device pair or the forms have the same ones ----

#define SET_DEVICE(c) DBGSOM_HIP_CHECK(hipSetDevice((c)->device))

// the masked, Manhattan and cosine search (k = 1 or 2)
int raw_bmu_checked(const char *fn, dbgsom_ctx *c, RowsForm form, const QueryRows &q, int x_dtype, int64_t Nq, int64_t d,
                    const double *W_host, int64_t M, int k, int64_t *idx_out, double *dist_out, void *Xfilled_host) {
    if (!c) { set_error("%s: null context", fn); return DBGSOM_EINVAL; }
    TRY(masked_check_shape(x_dtype, Nq, d, q.ldx, M, k));
    if (Nq == 0) return DBGSOM_OK;
    REQUIRE_FN(fn, q.p && W_host && idx_out && dist_out, "null pointer");
    SET_DEVICE(c);
    return raw_rows_query(c, fn, Q_BMU, form, q, x_dtype, Nq, d, W_host, M, k, idx_out, dist_out, 0, Xfilled_host);
}

// their distance matrix (rows of the result ldo apart; k = 1) and k nearest prototypes
int raw_rows_checked(const char *fn, dbgsom_ctx *c, QueryOp op, RowsForm form, const QueryRows &q, int x_dtype, int64_t Nq, int64_t d,
                     const double *W_host, int64_t M, int k, int64_t *idx_out, double *dist_out, int64_t ldo) {
    TRY(query_args(fn, c, op, x_dtype, true, Nq, d, M, k));
    TRY(masked_check_shape(x_dtype, Nq, d, q.ldx, M, 1));
    if (op == Q_DISTANCES) REQUIRE_FN(fn, ldo >= M, "ldo must be >= M");
    if (Nq == 0) return DBGSOM_OK;
    REQUIRE_FN(fn, q.p && W_host && (op == Q_DISTANCES || idx_out) && dist_out, "null pointer");
    SET_DEVICE(c);
    return raw_rows_query(c, fn, op, form, q, x_dtype, Nq, d, W_host, M, k, idx_out, dist_out, ldo, nullptr);
}

// every Euclidean query of dense rows (csr == nullptr) or host CSR rows
int placed_rows_checked(const char *fn, dbgsom_ctx *c, PlacedQuery p, const QueryRows &q, const CsrHost *csr, int64_t Nq,
                        const double *W_host) {
    const QueryOp op = p.op;
    TRY(query_args(fn, c, op, p.x_dtype, csr != nullptr, Nq, p.d, p.M, p.k));
    // (an op that does not take an operand leaves it at its default, which passes)
    REQUIRE_FN(fn, p.n_values >= 0 && p.n_values <= DBGSOM_MAX_MIXTURE_VALUES, "need 0 <= n_values <= DBGSOM_MAX_MIXTURE_VALUES");
    REQUIRE_FN(fn, p.c >= 0.0, "c must be >= 0");   // (NaN fails)
    REQUIRE_FN(fn, p.E >= 0 && p.E <= 0x7fffffff, "need 0 <= E < 2^31");
    if (q.on_device) REQUIRE_FN(fn, q.ldx >= p.d, "ldx must be >= d");
    if (op == Q_DISTANCES) REQUIRE_FN(fn, p.ldo >= p.M, "ldo must be >= M");
    if (csr) {
        REQUIRE_FN(fn, csr->indptr && csr->nnz >= 0 && (csr->nnz == 0 || (csr->indices && q.p)), "bad arguments");
        TRY(dbgsom_csr_check(csr->indptr, csr->indices, Nq, p.d, csr->nnz));
    }
    if (Nq == 0) return DBGSOM_OK;
    REQUIRE_FN(fn, (csr || q.p) && W_host && (op == Q_DISTANCES || p.idx_out) && (op == Q_RANGE_COUNTS || p.res_out),
               "null pointer");
    REQUIRE_FN(fn, (op != Q_RANGE_COUNTS || p.thr_host) && (op != Q_DISTORTION || p.H_host) && (p.E == 0 || p.edges_host) &&
                       (op != Q_MIXTURE || (p.logprior_host && (p.n_values == 0 || (p.Y_host && p.q_out)))), "null pointer");
    SET_DEVICE(c);
    return placed_rows_query(c, p, q, csr, Nq, W_host);
}

}  // namespace

// ------------------------------------------------------------------------------------------
// query rows with missing entries (NaN): csrc/masked.hip and the masked forms of distances.hip / kneighbors.hip
// ------------------------------------------------------------------------------------------
int dbgsom_ctx_bmu_query_masked(dbgsom_ctx *c, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d,
                                const double *W_host, int64_t M, int k, int64_t *idx_host, double *dist_host,
                                void *Xfilled_host) {
    return raw_bmu_checked(__func__, c, ROWS_MASKED, QueryRows{Xq_host, false, d}, x_dtype, Nq, d, W_host, M, k, idx_host,
                           dist_host, Xfilled_host);
}

int dbgsom_ctx_distances_query_masked(dbgsom_ctx *c, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d,
                                      const double *W_host, int64_t M, double *out_host) {
    return raw_rows_checked(__func__, c, Q_DISTANCES, ROWS_MASKED, QueryRows{Xq_host, false, d}, x_dtype, Nq, d, W_host, M,
                            1, nullptr, out_host, M);
}

int dbgsom_ctx_kneighbors_query_masked(dbgsom_ctx *c, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d,
                                       const double *W_host, int64_t M, int k, int64_t *idx_host, double *dist_host) {
    return raw_rows_checked(__func__, c, Q_KNEIGHBORS, ROWS_MASKED, QueryRows{Xq_host, false, d}, x_dtype, Nq, d, W_host, M,
                            k, idx_host, dist_host, 0);
}

// ------------------------------------------------------------------------------------------
// the Euclidean distance matrix and k nearest prototypes of a query: csrc/distances.hip, csrc/kneighbors.hip
// ------------------------------------------------------------------------------------------
int dbgsom_ctx_distances_query(dbgsom_ctx *c, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d,
                               const double *W_host, int64_t M, double *out_host) {
    PlacedQuery p{Q_DISTANCES, x_dtype, d, M, 1, nullptr, out_host};
    p.ldo = M;
    return placed_rows_checked(__func__, c, p, QueryRows{Xq_host, false, d}, nullptr, Nq, W_host);
}

int dbgsom_ctx_distances_query_device(dbgsom_ctx *c, const void *Xq_dev, int x_dtype, int64_t Nq, int64_t d, int64_t ldx,
                                      const double *W_host, int64_t M, double *out_dev, int64_t ldo) {
    PlacedQuery p{Q_DISTANCES, x_dtype, d, M, 1, nullptr, out_dev};
    p.ldo = ldo;
    return placed_rows_checked(__func__, c, p, QueryRows{Xq_dev, true, ldx}, nullptr, Nq, W_host);
}

int dbgsom_ctx_distances_query_csr(dbgsom_ctx *c, const int64_t *indptr_host, const int32_t *indices_host,
                                   const void *data_host, int x_dtype, int64_t Nq, int64_t d, int64_t nnz,
                                   const double *W_host, int64_t M, double *out_host) {
    const CsrHost csr{indptr_host, indices_host, nnz};
    PlacedQuery p{Q_DISTANCES, x_dtype, d, M, 1, nullptr, out_host};
    p.ldo = M;
    return placed_rows_checked(__func__, c, p, QueryRows{data_host, false, d}, &csr, Nq, W_host);
}

int dbgsom_ctx_kneighbors_query(dbgsom_ctx *c, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d,
                                const double *W_host, int64_t M, int k, int64_t *idx_host, double *dist_host) {
    const PlacedQuery p{Q_KNEIGHBORS, x_dtype, d, M, k, idx_host, dist_host};
    return placed_rows_checked(__func__, c, p, QueryRows{Xq_host, false, d}, nullptr, Nq, W_host);
}

int dbgsom_ctx_kneighbors_query_device(dbgsom_ctx *c, const void *Xq_dev, int x_dtype, int64_t Nq, int64_t d, int64_t ldx,
                                       const double *W_host, int64_t M, int k, int64_t *idx_dev, double *dist_dev) {
    const PlacedQuery p{Q_KNEIGHBORS, x_dtype, d, M, k, idx_dev, dist_dev};
    return placed_rows_checked(__func__, c, p, QueryRows{Xq_dev, true, ldx}, nullptr, Nq, W_host);
}

int dbgsom_ctx_kneighbors_query_csr(dbgsom_ctx *c, const int64_t *indptr_host, const int32_t *indices_host,
                                    const void *data_host, int x_dtype, int64_t Nq, int64_t d, int64_t nnz,
                                    const double *W_host, int64_t M, int k, int64_t *idx_host, double *dist_host) {
    const CsrHost csr{indptr_host, indices_host, nnz};
    const PlacedQuery p{Q_KNEIGHBORS, x_dtype, d, M, k, idx_host, dist_host};
    return placed_rows_checked(__func__, c, p, QueryRows{data_host, false, d}, &csr, Nq, W_host);
}

// ------------------------------------------------------------------------------------------
// the nearest resident rows of a query, through the partition: csrc/kneighbors.hip, csrc/row_neighbors.hip
// ------------------------------------------------------------------------------------------
namespace {

// what the scan needs of the context: dense float32 / float64 residents and the partition of dbgsom_ctx_partition on M units
int row_neighbors_state(const char *fn, const dbgsom_ctx *c, int64_t d, int64_t M) {
    TRY(loaded(c, fn));
    const char *why = nullptr;
    if (c->xs.csr) why = "the resident samples are CSR (load dense rows)";
    else if (c->xs.dtype == DBGSOM_BF16) why = "the resident samples are stored as bfloat16 (load them in their own dtype)";
    else if (!c->part_valid) why = "no valid partition of the resident samples (call dbgsom_ctx_partition after the load)";
    else if (c->partM != M) why = "M is not the partition's (call dbgsom_ctx_partition with these prototypes)";
    if (why) { set_error("%s: %s", fn, why); return DBGSOM_ESTATE; }
    REQUIRE_FN(fn, d == c->xs.d, "d must be the resident rows'");
    return DBGSOM_OK;
}

int row_neighbors_checked(const char *fn, dbgsom_ctx *c, const QueryRows &q, int q_dtype, int64_t Nq, int64_t d,
                          const double *W_host, int64_t M, int n_probe, int k, int64_t *idx_out, double *dist_out) {
    // (the scan's own argument checks need no context: they come first)
    TRY(scan_cells_check(fn, DBGSOM_F32, 0, d, d, M, q_dtype, Nq, q.ldx, n_probe, k));
    if (!c) { set_error("%s: null context", fn); return DBGSOM_EINVAL; }
    TRY(row_neighbors_state(fn, c, d, M));
    PlacedQuery p{Q_ROW_NEIGHBORS, q_dtype, d, M, k, idx_out, dist_out};
    p.n_probe = n_probe;
    return placed_rows_checked(fn, c, p, q, nullptr, Nq, W_host);
}

}  // namespace

int dbgsom_ctx_row_neighbors_query(dbgsom_ctx *c, const void *Q_host, int q_dtype, int64_t Nq, int64_t d,
                                   const double *W_host, int64_t M, int n_probe, int k, int64_t *idx_host,
                                   double *dist_host) {
    return row_neighbors_checked(__func__, c, QueryRows{Q_host, false, d}, q_dtype, Nq, d, W_host, M, n_probe, k, idx_host,
                                 dist_host);
}

int dbgsom_ctx_row_neighbors_query_device(dbgsom_ctx *c, const void *Q_dev, int q_dtype, int64_t Nq, int64_t d, int64_t ldq,
                                          const double *W_host, int64_t M, int n_probe, int k, int64_t *idx_dev,
                                          double *dist_dev) {
    return row_neighbors_checked(__func__, c, QueryRows{Q_dev, true, ldq}, q_dtype, Nq, d, W_host, M, n_probe, k, idx_dev,
                                 dist_dev);
}

int dbgsom_ctx_scan_cells_device(dbgsom_ctx *c, const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx,
                                 const int32_t *order_dev, const uint32_t *seg_start_dev, int64_t M, const void *Q_dev,
                                 int q_dtype, int64_t Nq, int64_t ldq, const int64_t *probe_dev, int n_probe, int k,
                                 int64_t *idx_dev, double *dist_dev) {
    TRY(scan_cells_check(__func__, x_dtype, N, d, ldx, M, q_dtype, Nq, ldq, n_probe, k));
    CTX_CHECK(c);
    if (Nq == 0) return DBGSOM_OK;
    return finish_query(c, launch_scan_cells(__func__, X_dev, x_dtype, N, d, ldx, order_dev, seg_start_dev, M, Q_dev, q_dtype,
                                             Nq, ldq, probe_dev, n_probe, k, idx_dev, dist_dev, c->stream));
}

// ------------------------------------------------------------------------------------------
// the distortion measure of a query: csrc/distortion.hip
// ------------------------------------------------------------------------------------------
int dbgsom_ctx_distortion_query(dbgsom_ctx *c, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d,
                                const double *W_host, int64_t M, const double *H_host, int64_t *bmu_host, double *e_host) {
    PlacedQuery p{Q_DISTORTION, x_dtype, d, M, 1, bmu_host, e_host};
    p.H_host = H_host;
    return placed_rows_checked(__func__, c, p, QueryRows{Xq_host, false, d}, nullptr, Nq, W_host);
}

int dbgsom_ctx_distortion_query_device(dbgsom_ctx *c, const void *Xq_dev, int x_dtype, int64_t Nq, int64_t d, int64_t ldx,
                                       const double *W_host, int64_t M, const double *H_host, int64_t *bmu_dev,
                                       double *e_dev) {
    PlacedQuery p{Q_DISTORTION, x_dtype, d, M, 1, bmu_dev, e_dev};
    p.H_host = H_host;
    return placed_rows_checked(__func__, c, p, QueryRows{Xq_dev, true, ldx}, nullptr, Nq, W_host);
}

int dbgsom_ctx_distortion_query_csr(dbgsom_ctx *c, const int64_t *indptr_host, const int32_t *indices_host,
                                    const void *data_host, int x_dtype, int64_t Nq, int64_t d, int64_t nnz,
                                    const double *W_host, int64_t M, const double *H_host, int64_t *bmu_host,
                                    double *e_host) {
    const CsrHost csr{indptr_host, indices_host, nnz};
    PlacedQuery p{Q_DISTORTION, x_dtype, d, M, 1, bmu_host, e_host};
    p.H_host = H_host;
    return placed_rows_checked(__func__, c, p, QueryRows{data_host, false, d}, &csr, Nq, W_host);
}

// ------------------------------------------------------------------------------------------
// the k nearest rows of a query to every prototype: csrc/exemplars.hip (idx / dist: M x k; Nq == 0 writes nothing)
// ------------------------------------------------------------------------------------------
int dbgsom_ctx_exemplars_query(dbgsom_ctx *c, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d, const double *W_host,
                               int64_t M, int k, int own_cell, int64_t *idx_host, double *dist_host) {
    PlacedQuery p{Q_EXEMPLARS, x_dtype, d, M, k, idx_host, dist_host};
    p.own_cell = own_cell;
    return placed_rows_checked(__func__, c, p, QueryRows{Xq_host, false, d}, nullptr, Nq, W_host);
}

int dbgsom_ctx_exemplars_query_device(dbgsom_ctx *c, const void *Xq_dev, int x_dtype, int64_t Nq, int64_t d, int64_t ldx,
                                      const double *W_host, int64_t M, int k, int own_cell, int64_t *idx_dev,
                                      double *dist_dev) {
    PlacedQuery p{Q_EXEMPLARS, x_dtype, d, M, k, idx_dev, dist_dev};
    p.own_cell = own_cell;
    return placed_rows_checked(__func__, c, p, QueryRows{Xq_dev, true, ldx}, nullptr, Nq, W_host);
}

int dbgsom_ctx_exemplars_query_csr(dbgsom_ctx *c, const int64_t *indptr_host, const int32_t *indices_host,
                                   const void *data_host, int x_dtype, int64_t Nq, int64_t d, int64_t nnz,
                                   const double *W_host, int64_t M, int k, int own_cell, int64_t *idx_host,
                                   double *dist_host) {
    const CsrHost csr{indptr_host, indices_host, nnz};
    PlacedQuery p{Q_EXEMPLARS, x_dtype, d, M, k, idx_host, dist_host};
    p.own_cell = own_cell;
    return placed_rows_checked(__func__, c, p, QueryRows{data_host, false, d}, &csr, Nq, W_host);
}

// ------------------------------------------------------------------------------------------
// the rows of a query within a radius of every prototype: csrc/density.hip (counts: M x n_radii; Nq == 0 writes nothing)
// ------------------------------------------------------------------------------------------
int dbgsom_ctx_range_counts_query(dbgsom_ctx *c, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d, const double *W_host,
                                  int64_t M, const double *thr_host, int n_radii, int64_t *counts_host) {
    PlacedQuery p{Q_RANGE_COUNTS, x_dtype, d, M, n_radii, counts_host, nullptr};
    p.thr_host = thr_host;
    return placed_rows_checked(__func__, c, p, QueryRows{Xq_host, false, d}, nullptr, Nq, W_host);
}

int dbgsom_ctx_range_counts_query_device(dbgsom_ctx *c, const void *Xq_dev, int x_dtype, int64_t Nq, int64_t d, int64_t ldx,
                                         const double *W_host, int64_t M, const double *thr_host, int n_radii,
                                         int64_t *counts_dev) {
    PlacedQuery p{Q_RANGE_COUNTS, x_dtype, d, M, n_radii, counts_dev, nullptr};
    p.thr_host = thr_host;
    return placed_rows_checked(__func__, c, p, QueryRows{Xq_dev, true, ldx}, nullptr, Nq, W_host);
}

int dbgsom_ctx_range_counts_query_csr(dbgsom_ctx *c, const int64_t *indptr_host, const int32_t *indices_host,
                                      const void *data_host, int x_dtype, int64_t Nq, int64_t d, int64_t nnz,
                                      const double *W_host, int64_t M, const double *thr_host, int n_radii,
                                      int64_t *counts_host) {
    const CsrHost csr{indptr_host, indices_host, nnz};
    PlacedQuery p{Q_RANGE_COUNTS, x_dtype, d, M, n_radii, counts_host, nullptr};
    p.thr_host = thr_host;
    return placed_rows_checked(__func__, c, p, QueryRows{data_host, false, d}, &csr, Nq, W_host);
}

// ------------------------------------------------------------------------------------------
// the map as a Gaussian mixture: csrc/mixture.hip (unit, lse: Nq values; q: Nq x n_values)
// ------------------------------------------------------------------------------------------
int dbgsom_ctx_mixture_query(dbgsom_ctx *c, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d, const double *W_host,
                             int64_t M, const double *logprior_host, double cc, const double *Y_host, int n_values,
                             int64_t *unit_host, double *lse_host, double *q_host) {
    PlacedQuery p{Q_MIXTURE, x_dtype, d, M, 1, unit_host, lse_host};
    p.logprior_host = logprior_host; p.c = cc; p.Y_host = Y_host; p.n_values = n_values; p.q_out = q_host;
    return placed_rows_checked(__func__, c, p, QueryRows{Xq_host, false, d}, nullptr, Nq, W_host);
}

int dbgsom_ctx_mixture_query_device(dbgsom_ctx *c, const void *Xq_dev, int x_dtype, int64_t Nq, int64_t d, int64_t ldx,
                                    const double *W_host, int64_t M, const double *logprior_host, double cc,
                                    const double *Y_host, int n_values, int64_t *unit_dev, double *lse_dev, double *q_dev) {
    PlacedQuery p{Q_MIXTURE, x_dtype, d, M, 1, unit_dev, lse_dev};
    p.logprior_host = logprior_host; p.c = cc; p.Y_host = Y_host; p.n_values = n_values; p.q_out = q_dev;
    return placed_rows_checked(__func__, c, p, QueryRows{Xq_dev, true, ldx}, nullptr, Nq, W_host);
}

int dbgsom_ctx_mixture_query_csr(dbgsom_ctx *c, const int64_t *indptr_host, const int32_t *indices_host,
                                 const void *data_host, int x_dtype, int64_t Nq, int64_t d, int64_t nnz, const double *W_host,
                                 int64_t M, const double *logprior_host, double cc, const double *Y_host, int n_values,
                                 int64_t *unit_host, double *lse_host, double *q_host) {
    const CsrHost csr{indptr_host, indices_host, nnz};
    PlacedQuery p{Q_MIXTURE, x_dtype, d, M, 1, unit_host, lse_host};
    p.logprior_host = logprior_host; p.c = cc; p.Y_host = Y_host; p.n_values = n_values; p.q_out = q_host;
    return placed_rows_checked(__func__, c, p, QueryRows{data_host, false, d}, &csr, Nq, W_host);
}

// ------------------------------------------------------------------------------------------
// weighted geodesics of the map and the combined error of a query: csrc/geodesics.hip
// ------------------------------------------------------------------------------------------
int dbgsom_ctx_geodesics(dbgsom_ctx *c, const double *W_host, int64_t M, int64_t d, const int32_t *edges_host, int64_t E,
                         double *G_host) {
    if (!c) { set_error("%s: null context", __func__); return DBGSOM_EINVAL; }
    DBGSOM_REQUIRE(M >= 1 && M <= DBGSOM_MAX_PROTOTYPES, "need 1 <= M <= DBGSOM_MAX_PROTOTYPES");
    DBGSOM_REQUIRE(d >= 1 && d <= 0x7fffffff, "bad prototype shape");
    DBGSOM_REQUIRE(E >= 0 && E <= 0x7fffffff, "need 0 <= E < 2^31");
    DBGSOM_REQUIRE(W_host && G_host && (E == 0 || edges_host), "null pointer");
    SET_DEVICE(c);
    DevBuf Wq, wwq;
    const int64_t dp = pad16(d);
    int rc = place_query_weights(c, Wq, wwq, W_host, M, d, dp);
    if (rc == DBGSOM_OK) rc = queue_geodesics(c, Wq.as<double>(), M, d, dp, edges_host, E, 0);
    if (rc == DBGSOM_OK) rc = geodesics_status(__func__, carve_geodesics(c, E).status, M, c->stream);
    if (rc == DBGSOM_OK) rc = download_rows(c, M, nullptr, nullptr, 0, G_host, c->ce_g.as<double>(), M);
    rc = finish_query(c, rc);
    Wq.release(); wwq.release();
    return rc;
}

int dbgsom_ctx_combined_error_query(dbgsom_ctx *c, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d,
                                    const double *W_host, int64_t M, const int32_t *edges_host, int64_t E,
                                    int64_t *idx2_host, double *e_host) {
    PlacedQuery p{Q_COMBINED, x_dtype, d, M, 2, idx2_host, e_host};
    p.edges_host = edges_host; p.E = E;
    return placed_rows_checked(__func__, c, p, QueryRows{Xq_host, false, d}, nullptr, Nq, W_host);
}

int dbgsom_ctx_combined_error_query_device(dbgsom_ctx *c, const void *Xq_dev, int x_dtype, int64_t Nq, int64_t d, int64_t ldx,
                                           const double *W_host, int64_t M, const int32_t *edges_host, int64_t E,
                                           int64_t *idx2_dev, double *e_dev) {
    PlacedQuery p{Q_COMBINED, x_dtype, d, M, 2, idx2_dev, e_dev};
    p.edges_host = edges_host; p.E = E;
    return placed_rows_checked(__func__, c, p, QueryRows{Xq_dev, true, ldx}, nullptr, Nq, W_host);
}

int dbgsom_ctx_combined_error_query_csr(dbgsom_ctx *c, const int64_t *indptr_host, const int32_t *indices_host,
                                        const void *data_host, int x_dtype, int64_t Nq, int64_t d, int64_t nnz,
                                        const double *W_host, int64_t M, const int32_t *edges_host, int64_t E,
                                        int64_t *idx2_host, double *e_host) {
    const CsrHost csr{indptr_host, indices_host, nnz};
    PlacedQuery p{Q_COMBINED, x_dtype, d, M, 2, idx2_host, e_host};
    p.edges_host = edges_host; p.E = E;
    return placed_rows_checked(__func__, c, p, QueryRows{data_host, false, d}, &csr, Nq, W_host);
}

// ------------------------------------------------------------------------------------------
// sparse coding (transform / predict_proba): csrc/sparse_code.hip, in chunks of query rows
// ------------------------------------------------------------------------------------------
// Rows from the host (q.on_device false): every chunk is staged in sc_x, coded into sc_code / sc_proba and copied to
// the host arrays code_host / proba_host.  Rows in HBM: the coder walks them where they are, q.ldx elements apart,
// and writes the caller's device arrays (code_host / proba_host are then device pointers) chunk by chunk.
static int sparse_code_impl(dbgsom_ctx *c, const QueryRows &q, int x_dtype, int64_t Nq, int64_t d,
                            const double *W_host, int64_t M, int max_iter, const double *P_host, int64_t C,
                            double *code_host, double *proba_host, uint64_t *counts_host) {
    const void *Xq_host = q.p;
    int64_t ldw = d;
    const double *Wd = nullptr;
    if (W_host) {
        TRY(c->sc_w.reserve((size_t)M * d * 8));
        DBGSOM_HIP_CHECK(hipMemcpyAsync(c->sc_w.p, W_host, (size_t)M * d * 8, hipMemcpyHostToDevice, c->stream));
        Wd = c->sc_w.as<double>();
    } else {
        if (c->M < 1 || c->xs.dtype < 0 || c->M != M || c->xs.d != d) {
            set_error("dbgsom_ctx_sparse_code: no resident prototypes of %lld x %lld rows; pass W_host",
                      (long long)M, (long long)d);
            return DBGSOM_ESTATE;
        }
        Wd = c->Wb[c->cur].as<double>();
        ldw = c->xs.dp;
    }
    TRY(c->sc_cnt.reserve(DBGSOM_SC_COUNTS * 8));
    DBGSOM_HIP_CHECK(hipMemsetAsync(c->sc_cnt.p, 0, DBGSOM_SC_COUNTS * 8, c->stream));
    if (proba_host) {
        TRY(c->sc_p.reserve((size_t)M * C * 8));
        DBGSOM_HIP_CHECK(hipMemcpyAsync(c->sc_p.p, P_host, (size_t)M * C * 8, hipMemcpyHostToDevice, c->stream));
    }
    const int64_t chunk = std::min<int64_t>(std::max<int64_t>(Nq, 1), c->sc_chunk_rows);
    const size_t es = dtype_size(x_dtype);
    TRY(c->sc_ws.reserve(dbgsom_sparse_code_workspace_bytes(chunk, d, M, max_iter)));
    if (q.on_device) {
        for (int64_t r0 = 0; r0 < Nq; r0 += chunk) {
            const int64_t n = std::min(chunk, Nq - r0);
            TRY(dbgsom_sparse_code(static_cast<const char *>(q.p) + (size_t)r0 * q.ldx * es, x_dtype, n, d, q.ldx, Wd, M, ldw,
                                   max_iter, (int)c->sc_cap, proba_host ? c->sc_p.as<double>() : nullptr, C,
                                   code_host ? code_host + r0 * M : nullptr, proba_host ? proba_host + r0 * C : nullptr,
                                   c->sc_cnt.as<uint64_t>(), c->sc_ws.p, c->sc_ws.cap, c->stream));
        }
        DBGSOM_HIP_CHECK(hipMemcpyAsync(counts_host, c->sc_cnt.p, DBGSOM_SC_COUNTS * 8, hipMemcpyDeviceToHost, c->stream));
        return sync(c);
    }
    TRY(c->sc_x.reserve((size_t)chunk * d * es));
    if (code_host) TRY(c->sc_code.reserve((size_t)chunk * M * 8));
    if (proba_host) TRY(c->sc_proba.reserve((size_t)chunk * C * 8));
    for (int64_t r0 = 0; r0 < Nq; r0 += chunk) {
        const int64_t n = std::min(chunk, Nq - r0);
        DBGSOM_HIP_CHECK(hipMemcpyAsync(c->sc_x.p, static_cast<const char *>(Xq_host) + (size_t)r0 * d * es,
                                        (size_t)n * d * es, hipMemcpyHostToDevice, c->stream));
        c->x_up((size_t)n * d * es);
        TRY(dbgsom_sparse_code(c->sc_x.p, x_dtype, n, d, d, Wd, M, ldw, max_iter, (int)c->sc_cap,
                               proba_host ? c->sc_p.as<double>() : nullptr, C,
                               code_host ? c->sc_code.as<double>() : nullptr,
                               proba_host ? c->sc_proba.as<double>() : nullptr, c->sc_cnt.as<uint64_t>(), c->sc_ws.p,
                               c->sc_ws.cap, c->stream));
        if (code_host) {
            DBGSOM_HIP_CHECK(hipMemcpyAsync(code_host + r0 * M, c->sc_code.p, (size_t)n * M * 8, hipMemcpyDeviceToHost,
                                            c->stream));
            c->x_down((size_t)n * M * 8);
        }
        if (proba_host) {
            DBGSOM_HIP_CHECK(hipMemcpyAsync(proba_host + r0 * C, c->sc_proba.p, (size_t)n * C * 8,
                                            hipMemcpyDeviceToHost, c->stream));
            c->x_down((size_t)n * C * 8);
        }
    }
    DBGSOM_HIP_CHECK(hipMemcpyAsync(counts_host, c->sc_cnt.p, DBGSOM_SC_COUNTS * 8, hipMemcpyDeviceToHost, c->stream));
    return sync(c);
}

int dbgsom_ctx_sparse_code(dbgsom_ctx *c, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d,
                           const double *W_host, int64_t M, int max_iter, const double *P_host, int64_t C,
                           double *code_host, double *proba_host, uint64_t *counts_host) {
    CTX_CHECK(c);
    DBGSOM_REQUIRE(x_dtype == DBGSOM_F32 || x_dtype == DBGSOM_F64, "x_dtype must be DBGSOM_F32 or DBGSOM_F64");
    DBGSOM_REQUIRE(counts_host && Nq >= 0 && d >= 1 && M >= 1 && max_iter >= 0 && (Nq == 0 || Xq_host),
                   "bad arguments");
    DBGSOM_REQUIRE(!proba_host || (P_host && C >= 1), "proba_host needs P_host and C >= 1");
    return sparse_code_impl(c, QueryRows{Xq_host, false, d}, x_dtype, Nq, d, W_host, M, max_iter, P_host, C, code_host,
                            proba_host, counts_host);
}

int dbgsom_ctx_sparse_code_device(dbgsom_ctx *c, const void *Xq_dev, int x_dtype, int64_t Nq, int64_t d, int64_t ldx,
                                  const double *W_host, int64_t M, int max_iter, const double *P_host, int64_t C,
                                  double *code_dev, double *proba_dev, uint64_t *counts_host) {
    CTX_CHECK(c);
    DBGSOM_REQUIRE(x_dtype == DBGSOM_F32 || x_dtype == DBGSOM_F64, "x_dtype must be DBGSOM_F32 or DBGSOM_F64");
    DBGSOM_REQUIRE(counts_host && Nq >= 0 && d >= 1 && ldx >= d && M >= 1 && max_iter >= 0 && (Nq == 0 || Xq_dev),
                   "bad arguments");
    DBGSOM_REQUIRE(!proba_dev || (P_host && C >= 1), "proba_dev needs P_host and C >= 1");
    return sparse_code_impl(c, QueryRows{Xq_dev, true, ldx}, x_dtype, Nq, d, W_host, M, max_iter, P_host, C, code_dev,
                            proba_dev, counts_host);
}

// ------------------------------------------------------------------------------------------
// topographic function: the k = 2 query search of dbgsom_ctx_bmu_query (k = 2 never takes the
// filtered form), its pairs left in HBM for csrc/topofn.hip
// ------------------------------------------------------------------------------------------
static int topographic_function_impl(dbgsom_ctx *c, const QueryRows &q, int x_dtype, int64_t Nq, int64_t d,
                                     const double *W_host, int64_t M, int round_f32, const int32_t *xy_host,
                                     int64_t n_pos, int64_t *hist_pos_host, int64_t *hist_neg_host, int32_t *D_host) {
    Samples &s = c->xq;
    DevBuf Wq, wwq, iq, dq, xy, hp, hn, Dd, ws;
    const bool timed = topofn_timing_enabled();
    hipEvent_t ev[2] = {nullptr, nullptr};
    int rc = DBGSOM_OK;
    const int64_t dp = pad16(d);
    do {
        if (timed) {
            hipError_t e = hipEventCreate(&ev[0]);
            if (e == hipSuccess) e = hipEventCreate(&ev[1]);
            if (e == hipSuccess) e = hipEventRecord(ev[0], c->stream);
            if (e != hipSuccess) { set_error("timing events: %s", hipGetErrorString(e)); rc = DBGSOM_EHIP; break; }
        }
        if ((rc = place_query_rows(c, s, q, x_dtype, Nq, d))) break;
        if ((rc = Wq.reserve((size_t)M * dp * 8))) break;
        if ((rc = wwq.reserve((size_t)M * 8))) break;
        if ((rc = iq.reserve((size_t)Nq * 2 * 8))) break;
        if ((rc = dq.reserve((size_t)Nq * 2 * 8))) break;
        if ((rc = upload_padded(c, Wq.p, W_host, M, d, dp, 8))) break;
        if ((rc = launch_row_sqnorms(Wq.p, DBGSOM_F64, M, dp, dp, wwq.as<double>(), c->stream))) break;
        if ((rc = launch_bmu(s.Xb, s.bdtype, Nq, dp, dp, s.xx.as<double>(), Wq.as<double>(), M, wwq.as<double>(), 2,
                             round_f32, iq.as<int64_t>(), dq.as<double>(), c->stream)))
            break;
        if (timed) {
            float ms = 0.0f;
            hipError_t e = hipEventRecord(ev[1], c->stream);
            if (e == hipSuccess) e = hipEventSynchronize(ev[1]);
            if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
            if (e != hipSuccess) { set_error("timing events: %s", hipGetErrorString(e)); rc = DBGSOM_EHIP; break; }
            topofn_add_search_ms(ms);
        }
        const size_t wsb = dbgsom_topofn_workspace_bytes(M, D_host != nullptr);
        if ((rc = xy.reserve((size_t)M * 8))) break;
        if ((rc = hp.reserve((size_t)n_pos * 8))) break;
        if ((rc = hn.reserve((size_t)(M + 1) * 8))) break;
        if ((rc = ws.reserve(wsb))) break;
        if (D_host && (rc = Dd.reserve((size_t)M * M * 4))) break;
        hipError_t e = hipMemcpyAsync(xy.p, xy_host, (size_t)M * 8, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) { set_error("H2D copy failed: %s", hipGetErrorString(e)); rc = DBGSOM_EHIP; break; }
        if ((rc = dbgsom_topofn(iq.as<int64_t>(), Nq, xy.as<int32_t>(), M, n_pos, hp.as<uint64_t>(),
                                hn.as<uint64_t>(), D_host ? Dd.as<int32_t>() : nullptr, ws.p, ws.cap, c->stream)))
            break;
        e = hipMemcpyAsync(hist_pos_host, hp.p, (size_t)n_pos * 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(hist_neg_host, hn.p, (size_t)(M + 1) * 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && D_host) e = hipMemcpyAsync(D_host, Dd.p, (size_t)M * M * 4, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) { set_error("D2H copy failed: %s", hipGetErrorString(e)); rc = DBGSOM_EHIP; }
    } while (0);
    if (rc != DBGSOM_OK) (void)hipStreamSynchronize(c->stream);
    for (hipEvent_t &e : ev)
        if (e) (void)hipEventDestroy(e);
    Wq.release(); wwq.release(); iq.release(); dq.release(); xy.release(); hp.release(); hn.release(); Dd.release();
    ws.release();
    drop_query_rows(s, q, Nq * dp * (int64_t)dtype_size(x_dtype));
    return rc;
}

int dbgsom_ctx_topographic_function(dbgsom_ctx *c, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d,
                                    const double *W_host, int64_t M, int round_f32, const int32_t *xy_host,
                                    int64_t n_pos, int64_t *hist_pos_host, int64_t *hist_neg_host, int32_t *D_host) {
    CTX_CHECK(c);
    DBGSOM_REQUIRE(x_dtype == DBGSOM_F32 || x_dtype == DBGSOM_F64, "x_dtype must be DBGSOM_F32 or DBGSOM_F64");
    DBGSOM_REQUIRE(Xq_host && W_host && xy_host && hist_pos_host && hist_neg_host && Nq >= 1 && d >= 1 && M >= 2 &&
                       M <= DBGSOM_MAX_PROTOTYPES && n_pos >= 1,
                   "bad arguments");
    return topographic_function_impl(c, QueryRows{Xq_host, false, d}, x_dtype, Nq, d, W_host, M, round_f32, xy_host, n_pos,
                                     hist_pos_host, hist_neg_host, D_host);
}

int dbgsom_ctx_topographic_function_device(dbgsom_ctx *c, const void *Xq_dev, int x_dtype, int64_t Nq, int64_t d,
                                           int64_t ldx, const double *W_host, int64_t M, int round_f32,
                                           const int32_t *xy_host, int64_t n_pos, int64_t *hist_pos_host,
                                           int64_t *hist_neg_host, int32_t *D_host) {
    CTX_CHECK(c);
    DBGSOM_REQUIRE(x_dtype == DBGSOM_F32 || x_dtype == DBGSOM_F64, "x_dtype must be DBGSOM_F32 or DBGSOM_F64");
    DBGSOM_REQUIRE(Xq_dev && ldx >= d && W_host && xy_host && hist_pos_host && hist_neg_host && Nq >= 1 && d >= 1 && M >= 2 &&
                       M <= DBGSOM_MAX_PROTOTYPES && n_pos >= 1,
                   "bad arguments");
    return topographic_function_impl(c, QueryRows{Xq_dev, true, ldx}, x_dtype, Nq, d, W_host, M, round_f32, xy_host, n_pos,
                                     hist_pos_host, hist_neg_host, D_host);
}

// ------------------------------------------------------------------------------------------
// fit on rows with missing entries: the resident masked search, and one epoch (masked.hip, masked_fit.hip, smooth.hip)
// ------------------------------------------------------------------------------------------
int dbgsom_ctx_bmu_masked(dbgsom_ctx *c, const double *W_host, int64_t M, int k, int64_t *idx_host, double *dist_host) {
    CTX_CHECK(c);
    TRY(masked_ready(c, __func__));
    DBGSOM_REQUIRE(W_host && idx_host && dist_host && (k == 1 || k == 2), "bad arguments");
    DBGSOM_REQUIRE(M >= k, "need k <= M");
    int rc = resident_bmu_masked(c, W_host, M, k);
    if (rc == DBGSOM_OK) {
        hipError_t e = hipMemcpyAsync(idx_host, c->mf_idx.p, (size_t)c->xs.N * k * 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(dist_host, c->mf_dist.p, (size_t)c->xs.N * k * 8, hipMemcpyDeviceToHost, c->stream);
        if (e != hipSuccess) { set_error("D2H copy failed: %s", hipGetErrorString(e)); rc = DBGSOM_EHIP; }
    }
    const hipError_t es = hipStreamSynchronize(c->stream);   // (W_host is pageable: never return with its copy in flight)
    if (rc == DBGSOM_OK && es != hipSuccess) { set_error("hipStreamSynchronize failed: %s", hipGetErrorString(es)); rc = DBGSOM_EHIP; }
    return rc;
}

int dbgsom_ctx_epoch_masked(dbgsom_ctx *c, const double *W_host, int64_t M, double gamma, double sigma, double *W_new_host,
                            double *change_total_host, double *errors_host, double *activations_host, int64_t *idx_host,
                            double *dist_host) {
    CTX_CHECK(c);
    TRY(masked_ready(c, __func__));
    DBGSOM_REQUIRE(W_host && W_new_host && change_total_host && errors_host && activations_host, "null pointer");
    DBGSOM_REQUIRE(M >= 1 && sigma > 0.0, "bad arguments");
    if (c->topoM != M) {
        set_error("dbgsom_ctx_epoch_masked: topology holds %lld neurons, weights %lld (call "
                  "dbgsom_ctx_set_topology after growth)", (long long)c->topoM, (long long)M);
        return DBGSOM_ESTATE;
    }
    Samples &s = c->xs;
    const int64_t N = s.N, d = s.d;
    int32_t status = 0;
    int rc = DBGSOM_OK;
    do {
        if ((rc = c->mf_kw.reserve((size_t)N * 8))) break;
        if ((rc = c->mf_sums.reserve((size_t)M * (3 * d + 2) * 8))) break;
        if ((rc = c->mf_acc_ws.reserve(accumulate_masked_workspace_bytes(N, d, M)))) break;
        if ((rc = c->mf_sm_ws.reserve(smooth_masked_workspace_bytes(M, d)))) break;
        if ((rc = c->mf_wn.reserve((size_t)M * d * 8))) break;
        if ((rc = c->mf_scal.reserve(256))) break;
        if ((rc = resident_bmu_masked(c, W_host, M, 1))) break;
        const int64_t *idx = c->mf_idx.as<int64_t>();
        const double *dist = c->mf_dist.as<double>();
        double *sums = c->mf_sums.as<double>();
        double *chg = c->mf_scal.as<double>();
        int32_t *st = reinterpret_cast<int32_t *>(c->mf_scal.as<char>() + 64);
        if ((rc = launch_exp_similarity(dist, N, gamma, c->mf_kw.as<double>(), c->stream))) break;
        if ((rc = launch_accumulate_masked(s.X, s.dtype, N, d, s.dp, idx, c->mf_kw.as<double>(), dist, M, sums, st,
                                           c->mf_acc_ws.p, c->mf_acc_ws.cap, c->stream)))
            break;
        if ((rc = launch_smooth_masked(sums, M, d, c->hop.as<float>(), sigma, c->mf_w.as<double>(), c->mf_wn.as<double>(), chg,
                                       c->mf_sm_ws.p, c->mf_sm_ws.cap, c->stream)))
            break;
        hipError_t e = hipMemcpyAsync(W_new_host, c->mf_wn.p, (size_t)M * d * 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(change_total_host, chg, 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&status, st, 4, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(activations_host, sums + 3 * M * d, (size_t)M * 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(errors_host, sums + 3 * M * d + M, (size_t)M * 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && idx_host) e = hipMemcpyAsync(idx_host, idx, (size_t)N * 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && dist_host) e = hipMemcpyAsync(dist_host, dist, (size_t)N * 8, hipMemcpyDeviceToHost, c->stream);
        if (e != hipSuccess) { set_error("D2H copy failed: %s", hipGetErrorString(e)); rc = DBGSOM_EHIP; }
    } while (0);
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (rc == DBGSOM_OK && es != hipSuccess) { set_error("hipStreamSynchronize failed: %s", hipGetErrorString(es)); rc = DBGSOM_EHIP; }
    if (rc == DBGSOM_OK && status) { set_error("dbgsom_ctx_epoch_masked: a winner outside [0, M)"); rc = DBGSOM_ERANGE; }
    return rc;
}

// ------------------------------------------------------------------------------------------
// metric="manhattan" (manhattan.hip) and metric="cosine" (cosine.hip and the cosine forms of the MFMA kernels): the
// search of the resident rows and one epoch on it, one body each for both metrics, and the queries (raw_rows_query)
// ------------------------------------------------------------------------------------------
namespace {

// the search of the resident rows under W (device, M rows ldw apart; cosine: ldw is the rows' dp)
int resident_bmu_metric(dbgsom_ctx *c, Metric metric, const double *W, int64_t ldw, int64_t M, int k, int64_t *idx,
                        double *dist) {
    if (metric == METRIC_MANHATTAN) return resident_bmu_manhattan(c, W, ldw, M, k, idx, dist);
    return resident_bmu_cosine(c, W, M, k, idx, dist);
}

// dbgsom_ctx_bmu_manhattan / dbgsom_ctx_bmu_cosine (`fn`).  The prototypes go up as each search reads them: M x d for
// the Manhattan one, padded to the rows' dp for the cosine one.
int metric_bmu(dbgsom_ctx *c, const char *fn, Metric metric, const double *W_host, int64_t M, int k, int64_t *idx_host,
               double *dist_host) {
    TRY(metric_ready(c, fn, metric));
    REQUIRE_FN(fn, W_host && idx_host && dist_host && (k == 1 || k == 2), "bad arguments");
    if (metric == METRIC_MANHATTAN) REQUIRE_FN(fn, M >= k, "need k <= M");
    else REQUIRE_FN(fn, M >= k && M <= 0x7fffff00, "need k <= M < 2^31");
    Samples &s = c->xs;
    const int64_t ldw = metric == METRIC_MANHATTAN ? s.d : s.dp;
    int rc = DBGSOM_OK;
    do {
        if ((rc = c->mk_w.reserve((size_t)M * ldw * 8))) break;
        if ((rc = c->qidx.reserve((size_t)s.N * k * 8))) break;
        if ((rc = c->qdist.reserve((size_t)s.N * k * 8))) break;
        if ((rc = upload_padded(c, c->mk_w.p, W_host, M, s.d, ldw, 8))) break;
        if ((rc = resident_bmu_metric(c, metric, c->mk_w.as<double>(), ldw, M, k, c->qidx.as<int64_t>(), c->qdist.as<double>())))
            break;
        hipError_t e = hipMemcpyAsync(idx_host, c->qidx.p, (size_t)s.N * k * 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(dist_host, c->qdist.p, (size_t)s.N * k * 8, hipMemcpyDeviceToHost, c->stream);
        if (e != hipSuccess) { set_error("D2H copy failed: %s", hipGetErrorString(e)); rc = DBGSOM_EHIP; break; }
        c->x_down((size_t)s.N * k * 16);
    } while (0);
    const hipError_t es = hipStreamSynchronize(c->stream);   // (W_host is pageable: never return with its copy in flight)
    if (rc == DBGSOM_OK && es != hipSuccess) { set_error("hipStreamSynchronize failed: %s", hipGetErrorString(es)); rc = DBGSOM_EHIP; }
    return rc;
}

// dbgsom_ctx_epoch_manhattan / dbgsom_ctx_epoch_cosine (`fn`): the metric's search of the resident rows in front of the
// ordinary sums and smoothing of dbgsom_ctx_epoch.  The winners are no seeds and the distances no bounds of a later
// Euclidean search: hint and bound are dropped, and the search policy is not consulted (neither metric has a filtered
// form).
int metric_epoch(dbgsom_ctx *c, const char *fn, Metric metric, const double *W_host, int64_t M, double gamma, double sigma,
                 int layout, double *W_new_host, double *change_total_host, double *errors_host, double *activations_host,
                 int64_t *idx_host, double *dist_host) {
    TRY(metric_ready(c, fn, metric));
    REQUIRE_FN(fn, W_host && W_new_host && change_total_host && errors_host && activations_host, "null pointer");
    REQUIRE_FN(fn, M >= 1 && sigma > 0.0, "bad arguments");
    REQUIRE_FN(fn, layout == DBGSOM_CENTRES_COMPACT || layout == DBGSOM_CENTRES_ALIGNED, "bad layout");
    if (c->topoM != M) {
        set_error("%s: topology holds %lld neurons, weights %lld (call dbgsom_ctx_set_topology after growth)", fn,
                  (long long)c->topoM, (long long)M);
        return DBGSOM_ESTATE;
    }
    Samples &s = c->xs;
    int rc = DBGSOM_OK;
    do {
        if ((rc = stage_weights(c, W_host, M, s.d, s.dp))) break;
        if ((rc = c->idx[0].reserve((size_t)s.N * 8))) break;
        if ((rc = c->idx[1].reserve((size_t)s.N * 8))) break;
        if ((rc = c->dist.reserve((size_t)s.N * 8))) break;
        int64_t *idx = c->idx[c->icur ^ 1].as<int64_t>();
        c->last_filtered = false;
        c->search.foreign_search_begun();
        if ((rc = resident_bmu_metric(c, metric, c->Wb[c->cur].as<double>(), s.dp, M, 1, idx, c->dist.as<double>()))) break;
        c->icur ^= 1;
        c->search.foreign_search_done();
        if ((rc = accumulate_and_reduce(c, idx, nullptr, gamma, c->dist.as<double>(), M))) break;
        rc = smooth_and_fetch(c, M, sigma, layout, 0, W_new_host, change_total_host, errors_host, activations_host, idx,
                              idx_host, dist_host);
    } while (0);
    if (rc != DBGSOM_OK && rc != DBGSOM_ERANGE) (void)hipStreamSynchronize(c->stream);
    return rc;
}

}  // namespace

int dbgsom_ctx_bmu_manhattan(dbgsom_ctx *c, const double *W_host, int64_t M, int k, int64_t *idx_host, double *dist_host) {
    CTX_CHECK(c);
    return metric_bmu(c, __func__, METRIC_MANHATTAN, W_host, M, k, idx_host, dist_host);
}

int dbgsom_ctx_bmu_cosine(dbgsom_ctx *c, const double *W_host, int64_t M, int k, int64_t *idx_host, double *dist_host) {
    CTX_CHECK(c);
    return metric_bmu(c, __func__, METRIC_COSINE, W_host, M, k, idx_host, dist_host);
}

int dbgsom_ctx_epoch_manhattan(dbgsom_ctx *c, const double *W_host, int64_t M, double gamma, double sigma, int layout,
                               double *W_new_host, double *change_total_host, double *errors_host,
                               double *activations_host, int64_t *idx_host, double *dist_host) {
    CTX_CHECK(c);
    return metric_epoch(c, __func__, METRIC_MANHATTAN, W_host, M, gamma, sigma, layout, W_new_host, change_total_host,
                        errors_host, activations_host, idx_host, dist_host);
}

int dbgsom_ctx_epoch_cosine(dbgsom_ctx *c, const double *W_host, int64_t M, double gamma, double sigma, int layout,
                            double *W_new_host, double *change_total_host, double *errors_host,
                            double *activations_host, int64_t *idx_host, double *dist_host) {
    CTX_CHECK(c);
    return metric_epoch(c, __func__, METRIC_COSINE, W_host, M, gamma, sigma, layout, W_new_host, change_total_host,
                        errors_host, activations_host, idx_host, dist_host);
}

// the queries of both metrics: host rows, and rows in HBM (*_device: ldx elements apart, results in device arrays)
int dbgsom_ctx_bmu_query_manhattan(dbgsom_ctx *c, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d,
                                   const double *W_host, int64_t M, int k, int64_t *idx_host, double *dist_host) {
    return raw_bmu_checked(__func__, c, ROWS_MANHATTAN, QueryRows{Xq_host, false, d}, x_dtype, Nq, d, W_host, M, k,
                           idx_host, dist_host, nullptr);
}

int dbgsom_ctx_bmu_query_manhattan_device(dbgsom_ctx *c, const void *Xq_dev, int x_dtype, int64_t Nq, int64_t d, int64_t ldx,
                                          const double *W_host, int64_t M, int k, int64_t *idx_dev, double *dist_dev) {
    return raw_bmu_checked(__func__, c, ROWS_MANHATTAN, QueryRows{Xq_dev, true, ldx}, x_dtype, Nq, d, W_host, M, k, idx_dev,
                           dist_dev, nullptr);
}

int dbgsom_ctx_distances_query_manhattan(dbgsom_ctx *c, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d,
                                         const double *W_host, int64_t M, double *out_host) {
    return raw_rows_checked(__func__, c, Q_DISTANCES, ROWS_MANHATTAN, QueryRows{Xq_host, false, d}, x_dtype, Nq, d, W_host,
                            M, 1, nullptr, out_host, M);
}

int dbgsom_ctx_distances_query_manhattan_device(dbgsom_ctx *c, const void *Xq_dev, int x_dtype, int64_t Nq, int64_t d,
                                                int64_t ldx, const double *W_host, int64_t M, double *out_dev, int64_t ldo) {
    return raw_rows_checked(__func__, c, Q_DISTANCES, ROWS_MANHATTAN, QueryRows{Xq_dev, true, ldx}, x_dtype, Nq, d, W_host,
                            M, 1, nullptr, out_dev, ldo);
}

int dbgsom_ctx_kneighbors_query_manhattan(dbgsom_ctx *c, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d,
                                          const double *W_host, int64_t M, int k, int64_t *idx_host, double *dist_host) {
    return raw_rows_checked(__func__, c, Q_KNEIGHBORS, ROWS_MANHATTAN, QueryRows{Xq_host, false, d}, x_dtype, Nq, d, W_host,
                            M, k, idx_host, dist_host, 0);
}

int dbgsom_ctx_kneighbors_query_manhattan_device(dbgsom_ctx *c, const void *Xq_dev, int x_dtype, int64_t Nq, int64_t d,
                                                 int64_t ldx, const double *W_host, int64_t M, int k, int64_t *idx_dev,
                                                 double *dist_dev) {
    return raw_rows_checked(__func__, c, Q_KNEIGHBORS, ROWS_MANHATTAN, QueryRows{Xq_dev, true, ldx}, x_dtype, Nq, d, W_host,
                            M, k, idx_dev, dist_dev, 0);
}

int dbgsom_ctx_bmu_query_cosine(dbgsom_ctx *c, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d,
                                const double *W_host, int64_t M, int k, int64_t *idx_host, double *dist_host) {
    return raw_bmu_checked(__func__, c, ROWS_COSINE, QueryRows{Xq_host, false, d}, x_dtype, Nq, d, W_host, M, k, idx_host,
                           dist_host, nullptr);
}

int dbgsom_ctx_bmu_query_cosine_device(dbgsom_ctx *c, const void *Xq_dev, int x_dtype, int64_t Nq, int64_t d, int64_t ldx,
                                       const double *W_host, int64_t M, int k, int64_t *idx_dev, double *dist_dev) {
    return raw_bmu_checked(__func__, c, ROWS_COSINE, QueryRows{Xq_dev, true, ldx}, x_dtype, Nq, d, W_host, M, k, idx_dev,
                           dist_dev, nullptr);
}

int dbgsom_ctx_distances_query_cosine(dbgsom_ctx *c, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d,
                                      const double *W_host, int64_t M, double *out_host) {
    return raw_rows_checked(__func__, c, Q_DISTANCES, ROWS_COSINE, QueryRows{Xq_host, false, d}, x_dtype, Nq, d, W_host, M,
                            1, nullptr, out_host, M);
}

int dbgsom_ctx_distances_query_cosine_device(dbgsom_ctx *c, const void *Xq_dev, int x_dtype, int64_t Nq, int64_t d,
                                             int64_t ldx, const double *W_host, int64_t M, double *out_dev, int64_t ldo) {
    return raw_rows_checked(__func__, c, Q_DISTANCES, ROWS_COSINE, QueryRows{Xq_dev, true, ldx}, x_dtype, Nq, d, W_host, M,
                            1, nullptr, out_dev, ldo);
}

int dbgsom_ctx_kneighbors_query_cosine(dbgsom_ctx *c, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d,
                                       const double *W_host, int64_t M, int k, int64_t *idx_host, double *dist_host) {
    return raw_rows_checked(__func__, c, Q_KNEIGHBORS, ROWS_COSINE, QueryRows{Xq_host, false, d}, x_dtype, Nq, d, W_host, M,
                            k, idx_host, dist_host, 0);
}

int dbgsom_ctx_kneighbors_query_cosine_device(dbgsom_ctx *c, const void *Xq_dev, int x_dtype, int64_t Nq, int64_t d,
                                              int64_t ldx, const double *W_host, int64_t M, int k, int64_t *idx_dev,
                                              double *dist_dev) {
    return raw_rows_checked(__func__, c, Q_KNEIGHBORS, ROWS_COSINE, QueryRows{Xq_dev, true, ldx}, x_dtype, Nq, d, W_host, M,
                            k, idx_dev, dist_dev, 0);
}

int dbgsom_ctx_exp_similarity(dbgsom_ctx *c, const double *dist_host, int64_t n, double gamma, double *kw_host) {

    CTX_CHECK(c);
    DBGSOM_REQUIRE(n >= 0 && (n == 0 || (dist_host && kw_host)), "bad arguments");
    if (n == 0) return DBGSOM_OK;
    TRY(c->stage_dev.reserve((size_t)2 * n * 8));
    double *din = c->stage_dev.as<double>(), *dout = din + n;
    DBGSOM_HIP_CHECK(hipMemcpyAsync(din, dist_host, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    TRY(launch_exp_similarity(din, n, gamma, dout, c->stream));
    DBGSOM_HIP_CHECK(hipMemcpyAsync(kw_host, dout, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    return sync(c);
}

// ------------------------------------------------------------------------------------------
// the epoch
// ------------------------------------------------------------------------------------------
int dbgsom_ctx_epoch(dbgsom_ctx *c, const double *W_host, int64_t M, int round_f32, double gamma, double sigma,
                     int layout, int flags, double *W_new_host, double *change_total_host, double *errors_host,
                     double *activations_host, int64_t *idx_host, double *dist_host) {
    CTX_CHECK(c);
    TRY(loaded(c, __func__));
    TRY(complete_rows(c, __func__));
    DBGSOM_REQUIRE(change_total_host && errors_host && activations_host, "null output");
    DBGSOM_REQUIRE(layout == DBGSOM_CENTRES_COMPACT || layout == DBGSOM_CENTRES_ALIGNED, "bad layout");
    if (c->topoM != M) {
        set_error("dbgsom_ctx_epoch: topology holds %lld neurons, weights %lld (call "
                  "dbgsom_ctx_set_topology after growth)", (long long)c->topoM, (long long)M);
        return DBGSOM_ESTATE;
    }
    Samples &s = c->xs;
    int rc = DBGSOM_OK;
    do {
        if ((rc = stage_weights(c, W_host, M, s.d, s.dp))) break;
        mark(c, 0);
        const auto t_begin = std::chrono::steady_clock::now();
        c->anchor.begin_epoch();
        if ((rc = epoch_bmu(c, M, round_f32))) break;
        mark(c, 1);
        const int measuring = c->policy.take_timing_form();   // (the refinement's policy: this epoch times one of the two forms)
        const int64_t *idx = c->idx[c->icur].as<int64_t>();
        if ((rc = accumulate_and_reduce(c, idx, nullptr, gamma, c->dist.as<double>(), M))) break;
        // the next epoch's filter visits the samples bucketed by this epoch's winners: the stable
        // counting sort the accumulate step just did (first N int32 of its workspace)
        c->search.sums_made(M);
        mark(c, 2);
        rc = smooth_and_fetch(c, M, sigma, layout, flags, W_new_host, change_total_host, errors_host, activations_host,
                              idx, idx_host, dist_host);
        if (rc != DBGSOM_OK && rc != DBGSOM_ERANGE) break;
        SearchPolicy &pol = c->policy;
        if (measuring >= 0)   // wall clock of the blocking call behind the upload of W: BMU + sums + smoothing
            pol.refine_timed(measuring, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count());
        if (c->last_filtered) {
            const double *counted = c->tail.as<double>() + 2 * M + 2;   // (pack_results_kernel: lists, probe, groups to re-seed, handed over)
            // the lean gate's record, the clock's verdict and the valve of the anchor seeds: AnchorControl
            const AnchorControl::Verdict v = c->anchor.after_filtered_epoch(counted, s.N, M, s.anchor_generation, pol, measuring,
                                                                            W_new_host || idx_host || dist_host);
            const double epoch_ms =
                v.clean ? std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count() : NAN;
            if (v.drop_anchors) s.drop_anchors(2);
            pol.observe(counted[0], counted[1], counted[2], (s.N + 127) / 128, M, s.dp, (flags & DBGSOM_EPOCH_FROZEN) != 0,
                        epoch_ms);
        } else {
            c->anchor.after_unfiltered_epoch();
            pol.observe_unfiltered();
        }
    } while (0);
    if (rc != DBGSOM_OK && rc != DBGSOM_ERANGE) { (void)hipStreamSynchronize(c->stream); c->search.epoch_failed(); }
    return rc;
}

int dbgsom_ctx_update(dbgsom_ctx *c, const double *W_host, int64_t M, const int64_t *idx_host, const double *kw_host,
                      const double *dist_host, double sigma, int layout, double *W_new_host,
                      double *change_total_host, double *errors_host, double *activations_host) {
    CTX_CHECK(c);
    TRY(loaded(c, __func__));
    TRY(complete_rows(c, __func__));
    DBGSOM_REQUIRE(idx_host && kw_host && dist_host && change_total_host && errors_host && activations_host, "null pointer");
    DBGSOM_REQUIRE(layout == DBGSOM_CENTRES_COMPACT || layout == DBGSOM_CENTRES_ALIGNED, "bad layout");
    Samples &s = c->xs;
    int rc = DBGSOM_OK;
    do {
        if ((rc = stage_weights(c, W_host, M, s.d, s.dp))) break;
        if ((rc = c->idx[0].reserve((size_t)s.N * 8))) break;
        if ((rc = c->idx[1].reserve((size_t)s.N * 8))) break;
        if ((rc = c->dist.reserve((size_t)s.N * 8))) break;
        if ((rc = c->kw.reserve((size_t)s.N * 8))) break;
        c->search.foreign_search_begun();  // (the caller's distances: nothing a bound may rest on)
        c->icur ^= 1;
        int64_t *idx = c->idx[c->icur].as<int64_t>();
        hipError_t e = hipMemcpyAsync(idx, idx_host, (size_t)s.N * 8, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(c->kw.p, kw_host, (size_t)s.N * 8, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(c->dist.p, dist_host, (size_t)s.N * 8, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) { set_error("H2D copy failed: %s", hipGetErrorString(e)); rc = DBGSOM_EHIP; break; }
        c->last_filtered = false;
        c->search.caller_winners_taken();
        if ((rc = accumulate_and_reduce(c, idx, c->kw.as<double>(), 0.0, c->dist.as<double>(), M))) break;
        rc = smooth_and_fetch(c, M, sigma, layout, 0, W_new_host, change_total_host, errors_host, activations_host, idx,
                              nullptr, nullptr);
    } while (0);
    if (rc != DBGSOM_OK && rc != DBGSOM_ERANGE) (void)hipStreamSynchronize(c->stream);
    return rc;
}

int dbgsom_ctx_set_hint(dbgsom_ctx *c, const int64_t *idx_host, int64_t M) {
    CTX_CHECK(c);
    TRY(loaded(c, __func__));
    TRY(complete_rows(c, __func__));
    DBGSOM_REQUIRE(idx_host && M >= 1 && M <= DBGSOM_MAX_PROTOTYPES, "bad arguments");
    Samples &s = c->xs;
    for (int64_t i = 0; i < s.N; ++i) DBGSOM_REQUIRE(idx_host[i] >= 0 && idx_host[i] < M, "seed index out of range");
    TRY(c->idx[0].reserve((size_t)s.N * 8));
    TRY(c->idx[1].reserve((size_t)s.N * 8));
    // the bucket order lives where the accumulate step leaves it: the first N int32 of its workspace
    TRY(c->acc_ws.reserve(acc_ws_bytes(c, M)));
    TRY(c->part_ws.reserve(bucket_sort_workspace_bytes(s.N, M)));
    int64_t *idx = c->idx[c->icur].as<int64_t>();
    DBGSOM_HIP_CHECK(hipMemcpyAsync(idx, idx_host, (size_t)s.N * 8, hipMemcpyHostToDevice, c->stream));
    TRY(launch_bucket_sort(idx, s.N, M, c->acc_ws.as<int32_t>(), c->part_ws.p, c->stream));
    TRY(sync(c));
    c->search.hint_seeded(M);
    c->part_valid = false;
    return DBGSOM_OK;
}

int dbgsom_ctx_read_sums(dbgsom_ctx *c, double *sums_host, int64_t M) {
    CTX_CHECK(c);
    TRY(loaded(c, __func__));
    DBGSOM_REQUIRE(sums_host, "null pointer");
    if (c->sumsM != M || M < 1) { set_error("dbgsom_ctx_read_sums: no sums of %lld neurons", (long long)M); return DBGSOM_ESTATE; }
    const int64_t d = c->xs.d, dp = c->xs.dp;
    TRY(download_unpadded(c, sums_host, c->sums.p, M, d, dp, 8));
    DBGSOM_HIP_CHECK(hipMemcpyAsync(sums_host + M * d, c->sums.as<double>() + M * dp, (size_t)3 * M * 8,
                                    hipMemcpyDeviceToHost, c->stream));
    return sync(c);
}

// ------------------------------------------------------------------------------------------
// reductions around the path
// ------------------------------------------------------------------------------------------
int dbgsom_ctx_column_sums(dbgsom_ctx *c, const void *mean_host, void *out_host) {
    CTX_CHECK(c);
    TRY(loaded(c, __func__));
    TRY(complete_rows(c, __func__));
    DBGSOM_REQUIRE(out_host, "null pointer");
    Samples &s = c->xs;
    if (s.csr) { set_error("dbgsom_ctx_column_sums: the resident samples are CSR (take the column moments from the stored entries on the host)"); return DBGSOM_ESTATE; }
    DBGSOM_REQUIRE(s.dtype == DBGSOM_F32 || s.dtype == DBGSOM_F64, "float32 / float64 resident samples only");
    const size_t es = dtype_size(s.dtype);
    TRY(c->stage_dev.reserve((size_t)2 * s.dp * es + 512));
    char *mean_dev = c->stage_dev.as<char>();
    char *out_dev = mean_dev + align_up((size_t)s.dp * es);
    if (mean_host) {
        DBGSOM_HIP_CHECK(hipMemsetAsync(mean_dev, 0, (size_t)s.dp * es, c->stream));
        DBGSOM_HIP_CHECK(hipMemcpyAsync(mean_dev, mean_host, (size_t)s.d * es, hipMemcpyHostToDevice, c->stream));
    }
    TRY(dbgsom_column_sums(s.X, s.dtype, s.N, s.dp, s.dp, mean_host ? mean_dev : nullptr, out_dev, c->stream));
    DBGSOM_HIP_CHECK(hipMemcpyAsync(out_host, out_dev, (size_t)s.d * es, hipMemcpyDeviceToHost, c->stream));
    return sync(c);
}

int dbgsom_ctx_weighted_column_sums(dbgsom_ctx *c, const double *mean_host, double *out_host) {
    CTX_CHECK(c);
    TRY(loaded(c, __func__));
    TRY(complete_rows(c, __func__));
    DBGSOM_REQUIRE(out_host, "null pointer");
    if (!c->has_weights) { set_error("weighted column sums requested but no weights attached (dbgsom_ctx_set_sample_weight)"); return DBGSOM_ESTATE; }
    Samples &s = c->xs;
    if (s.csr) { set_error("dbgsom_ctx_weighted_column_sums: the resident samples are CSR (take the column moments from the stored entries on the host)"); return DBGSOM_ESTATE; }
    const size_t vec = align_up((size_t)s.dp * 8);
    TRY(c->stage_dev.reserve(2 * vec + dbgsom_weighted_column_sums_workspace_bytes(s.dp)));
    double *mean_dev = c->stage_dev.as<double>();
    double *out_dev = reinterpret_cast<double *>(c->stage_dev.as<char>() + vec);
    void *ws = c->stage_dev.as<char>() + 2 * vec;
    if (mean_host) {
        DBGSOM_HIP_CHECK(hipMemsetAsync(mean_dev, 0, (size_t)s.dp * 8, c->stream));
        DBGSOM_HIP_CHECK(hipMemcpyAsync(mean_dev, mean_host, (size_t)s.d * 8, hipMemcpyHostToDevice, c->stream));
    }
    TRY(dbgsom_weighted_column_sums(s.X, s.dtype, s.N, s.dp, s.dp, c->sw.as<double>(), mean_host ? mean_dev : nullptr, out_dev,
                                    ws, c->stage_dev.cap - 2 * vec, c->stream));
    DBGSOM_HIP_CHECK(hipMemcpyAsync(out_host, out_dev, (size_t)s.d * 8, hipMemcpyDeviceToHost, c->stream));
    return sync(c);
}

// Z = C^T (C V) and the column sums of C = X - mean over the resident rows (covariance.hip): what it needs is what the
// Manhattan and cosine calls need (metric_ready), in the same words
int dbgsom_ctx_covariance_apply(dbgsom_ctx *c, const double *mean_host, const double *V_host, int p, double *Z_host,
                                double *colsum_host) {
    CTX_CHECK(c);
    const char *fn = __func__;
    TRY(loaded(c, fn));
    if (c->xs.csr) { set_error("%s: CSR residents have no covariance pass", fn); return DBGSOM_EINVAL; }
    if (c->xs.dtype == DBGSOM_BF16) { set_error("%s: bfloat16 storage has no covariance pass", fn); return DBGSOM_EINVAL; }
    const char *why = nullptr;
    if (c->incomplete) why = "the resident rows have missing entries (option \"incomplete\")";
    else if (c->has_weights) why = "sample weights are attached";
    else if (c->coll_nranks > 1 || c->allreduce) why = "more than one rank";
    if (why) { set_error("%s: %s", fn, why); return DBGSOM_EINVAL; }
    DBGSOM_REQUIRE(p >= 1 && p <= DBGSOM_MAX_DIRECTIONS, "p must be 1 .. DBGSOM_MAX_DIRECTIONS");
    DBGSOM_REQUIRE(V_host && Z_host && colsum_host, "null pointer");
    Samples &s = c->xs;
    const size_t vec = align_up((size_t)s.d * 8), blk = align_up((size_t)s.d * p * 8);
    const size_t ws_bytes = dbgsom_covariance_apply_workspace_bytes(s.N, s.d, p);
    TRY(c->stage_dev.reserve(2 * vec + 2 * blk + ws_bytes));
    char *base = c->stage_dev.as<char>();
    double *mean_dev = reinterpret_cast<double *>(base), *colsum_dev = reinterpret_cast<double *>(base + vec);
    double *V_dev = reinterpret_cast<double *>(base + 2 * vec), *Z_dev = reinterpret_cast<double *>(base + 2 * vec + blk);
    void *ws = base + 2 * vec + 2 * blk;
    if (mean_host) DBGSOM_HIP_CHECK(hipMemcpyAsync(mean_dev, mean_host, (size_t)s.d * 8, hipMemcpyHostToDevice, c->stream));
    DBGSOM_HIP_CHECK(hipMemcpyAsync(V_dev, V_host, (size_t)s.d * p * 8, hipMemcpyHostToDevice, c->stream));
    c->x_up((size_t)s.d * (p + (mean_host ? 1 : 0)) * 8);
    TRY(dbgsom_covariance_apply(s.X, s.dtype, s.N, s.d, s.dp, mean_host ? mean_dev : nullptr, V_dev, p, Z_dev, colsum_dev,
                                ws, ws_bytes, c->stream));
    DBGSOM_HIP_CHECK(hipMemcpyAsync(Z_host, Z_dev, (size_t)s.d * p * 8, hipMemcpyDeviceToHost, c->stream));
    DBGSOM_HIP_CHECK(hipMemcpyAsync(colsum_host, colsum_dev, (size_t)s.d * 8, hipMemcpyDeviceToHost, c->stream));
    c->x_down((size_t)s.d * (p + 1) * 8);
    return sync(c);
}

static int reduce_small(dbgsom_ctx *c, double *buf_dev, int64_t n, double *out_host) {
    TRY(run_allreduce(c, buf_dev, n));
    DBGSOM_HIP_CHECK(hipMemcpyAsync(out_host, buf_dev, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    return sync(c);
}

int dbgsom_ctx_quantization_error(dbgsom_ctx *c, const double *W_host, int64_t M, int round_f32, double *out2) {
    CTX_CHECK(c);
    TRY(loaded(c, __func__));
    TRY(complete_rows(c, __func__));
    DBGSOM_REQUIRE(out2, "null pointer");
    TRY(resident_bmu(c, W_host, M, 1, round_f32));
    TRY(c->red.reserve(256 + dbgsom_sum_workspace_bytes()));
    double *r = c->red.as<double>();
    if (c->has_weights) {   // [sum w dist, sum w]
        TRY(dbgsom_weighted_sum_f64(c->qdist.as<double>(), c->sw.as<double>(), c->xs.N, r, c->red.as<char>() + 256,
                                    c->red.cap - 256, c->stream));
        TRY(dbgsom_weighted_sum_f64(nullptr, c->sw.as<double>(), c->xs.N, r + 1, c->red.as<char>() + 256, c->red.cap - 256,
                                    c->stream));
        return reduce_small(c, r, 2, out2);
    }
    TRY(dbgsom_sum_f64(c->qdist.as<double>(), c->xs.N, r, c->red.as<char>() + 256, c->red.cap - 256, c->stream));
    const double n = (double)c->xs.N;
    DBGSOM_HIP_CHECK(hipMemcpyAsync(r + 1, &n, 8, hipMemcpyHostToDevice, c->stream));
    return reduce_small(c, r, 2, out2);
}

int dbgsom_ctx_topographic_count(dbgsom_ctx *c, const double *W_host, int64_t M, int round_f32, const int32_t *xy_host,
                                 double *count_host) {
    CTX_CHECK(c);
    TRY(loaded(c, __func__));
    TRY(complete_rows(c, __func__));
    DBGSOM_REQUIRE(xy_host && count_host && M >= 2, "bad arguments");
    TRY(resident_bmu(c, W_host, M, 2, round_f32));
    TRY(c->red.reserve(256 + align_up((size_t)M * 8) + dbgsom_sum_workspace_bytes()));
    int32_t *xy = reinterpret_cast<int32_t *>(c->red.as<char>() + 256);
    DBGSOM_HIP_CHECK(hipMemcpyAsync(xy, xy_host, (size_t)M * 8, hipMemcpyHostToDevice, c->stream));
    if (c->has_weights) {   // the summed weight of such rows
        TRY(dbgsom_topographic_weight(c->qidx.as<int64_t>(), c->sw.as<double>(), c->xs.N, xy, M, c->red.as<double>(),
                                      c->red.as<char>() + 256 + align_up((size_t)M * 8), dbgsom_sum_workspace_bytes(), c->stream));
        return reduce_small(c, c->red.as<double>(), 1, count_host);
    }
    uint64_t *cnt = reinterpret_cast<uint64_t *>(c->red.as<char>() + 64);
    TRY(dbgsom_topographic_count(c->qidx.as<int64_t>(), c->xs.N, xy, M, cnt, c->stream));
    double *r = c->red.as<double>();
    hipLaunchKernelGGL(u64_to_f64_kernel, dim3(1), dim3(64), 0, c->stream, (const unsigned long long *)cnt, r, (int64_t)1);
    TRY(launch_status("u64_to_f64_kernel"));
    return reduce_small(c, r, 1, count_host);
}

int dbgsom_ctx_node_statistics(dbgsom_ctx *c, const double *W_host, int64_t M, int round_f32, double sigma,
                               double *hits_host, double *density_host) {
    CTX_CHECK(c);
    TRY(loaded(c, __func__));
    TRY(complete_rows(c, __func__));
    DBGSOM_REQUIRE(hits_host && density_host && sigma > 0.0, "bad arguments");
    Samples &s = c->xs;
    TRY(resident_bmu(c, W_host, M, 1, round_f32));
    TRY(c->kw.reserve((size_t)s.N * 8));
    TRY(dbgsom_density_terms(c->qdist.as<double>(), s.N, sigma, c->kw.as<double>(), c->stream));
    // K = density sums, a = hit counts of the fused buffer; the bucket order of the training hint is rewritten
    c->search.bucket_order_rewritten();
    DBGSOM_REQUIRE(M <= DBGSOM_MAX_PROTOTYPES, "M exceeds DBGSOM_MAX_PROTOTYPES");
    const int64_t count = M * (s.dp + 3);
    TRY(c->sums.reserve((size_t)(count + 1) * 8));
    TRY(c->acc_ws.reserve(acc_ws_bytes(c, M)));
    c->part_valid = false;
    c->sumsM = 0;
    if (s.csr)
        TRY(launch_accumulate_csr(s.view(), s.dtype, s.N, s.dp, c->qidx.as<int64_t>(), c->kw.as<double>(), 0.0,
                                  c->has_weights ? c->sw.as<double>() : nullptr, c->qdist.as<double>(), M,
                                  c->sums.as<double>(), nullptr, false, c->acc_ws.p, c->acc_ws.cap, c->stream));
    else if (c->has_weights)   // K = sum w term, a = sum w
        TRY(launch_accumulate_weighted(s.X, s.dtype, s.N, s.dp, s.dp, c->qidx.as<int64_t>(), c->kw.as<double>(),
                                       c->sw.as<double>(), c->qdist.as<double>(), M, c->sums.as<double>(), nullptr, c->acc_ws.p,
                                       c->acc_ws.cap, c->stream));
    else
        TRY(launch_accumulate(s.X, s.dtype, s.N, s.dp, s.dp, c->qidx.as<int64_t>(), c->kw.as<double>(), c->qdist.as<double>(), M,
                              c->sums.as<double>(), nullptr, c->acc_ws.p, c->acc_ws.cap, c->stream));
    double *tail = c->sums.as<double>() + M * s.dp;  // [K | a]
    TRY(run_allreduce(c, tail, 2 * M));
    DBGSOM_HIP_CHECK(hipMemcpyAsync(density_host, tail, (size_t)M * 8, hipMemcpyDeviceToHost, c->stream));
    DBGSOM_HIP_CHECK(hipMemcpyAsync(hits_host, tail + M, (size_t)M * 8, hipMemcpyDeviceToHost, c->stream));
    return sync(c);
}

int dbgsom_ctx_class_histogram(dbgsom_ctx *c, const int64_t *idx_host, int64_t n_classes, int64_t M, int64_t *hist_host) {
    CTX_CHECK(c);
    TRY(loaded(c, __func__));
    DBGSOM_REQUIRE(hist_host && n_classes >= 1 && M >= 1, "bad arguments");
    if (!c->has_labels) { set_error("class histogram requested but no labels attached (dbgsom_ctx_set_labels)"); return DBGSOM_ESTATE; }
    Samples &s = c->xs;
    const int64_t *idx = nullptr;
    if (idx_host) {
        TRY(c->qidx.reserve((size_t)s.N * 8));
        DBGSOM_HIP_CHECK(hipMemcpyAsync(c->qidx.p, idx_host, (size_t)s.N * 8, hipMemcpyHostToDevice, c->stream));
        idx = c->qidx.as<int64_t>();
    } else {
        if (!c->search.last_idx_valid) { set_error("no winners of a previous epoch in HBM"); return DBGSOM_ESTATE; }
        idx = c->idx[c->icur].as<int64_t>();
    }
    const int64_t n = M * n_classes;
    TRY(c->hist.reserve((size_t)2 * n * 8));
    uint64_t *h = c->hist.as<uint64_t>();
    double *hd = c->hist.as<double>() + n;
    TRY(dbgsom_class_histogram(idx, c->y.as<int32_t>(), s.N, M, n_classes, h, c->stream));
    hipLaunchKernelGGL(u64_to_f64_kernel, dim3(grid1d(n)), dim3(256), 0, c->stream, (const unsigned long long *)h, hd, n);
    TRY(launch_status("u64_to_f64_kernel"));
    TRY(run_allreduce(c, hd, n));
    std::vector<double> tmp;
    try { tmp.resize((size_t)n); } catch (...) { set_error("out of host memory"); return DBGSOM_ENOMEM; }
    DBGSOM_HIP_CHECK(hipMemcpyAsync(tmp.data(), hd, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    TRY(sync(c));
    for (int64_t e = 0; e < n; ++e) hist_host[e] = (int64_t)llround(tmp[(size_t)e]);
    return DBGSOM_OK;
}

// the weighted class histogram: hist[j, c] = sum of the weights of the rows of class c that chose neuron j, added in
// row order (a stable bucket sort of the winners, then one workgroup per neuron walks its list)
int dbgsom_ctx_class_histogram_weighted(dbgsom_ctx *c, const int64_t *idx_host, int64_t n_classes, int64_t M, double *hist_host) {
    CTX_CHECK(c);
    TRY(loaded(c, __func__));
    DBGSOM_REQUIRE(hist_host && n_classes >= 1 && M >= 1 && M <= DBGSOM_MAX_PROTOTYPES, "bad arguments");
    if (!c->has_labels) { set_error("class histogram requested but no labels attached (dbgsom_ctx_set_labels)"); return DBGSOM_ESTATE; }
    if (!c->has_weights) { set_error("weighted class histogram requested but no weights attached (dbgsom_ctx_set_sample_weight)"); return DBGSOM_ESTATE; }
    Samples &s = c->xs;
    const int64_t *idx = nullptr;
    if (idx_host) {
        TRY(c->qidx.reserve((size_t)s.N * 8));
        DBGSOM_HIP_CHECK(hipMemcpyAsync(c->qidx.p, idx_host, (size_t)s.N * 8, hipMemcpyHostToDevice, c->stream));
        idx = c->qidx.as<int64_t>();
    } else {
        if (!c->search.last_idx_valid) { set_error("no winners of a previous epoch in HBM"); return DBGSOM_ESTATE; }
        idx = c->idx[c->icur].as<int64_t>();
    }
    const int64_t n = M * n_classes;
    TRY(c->hist.reserve((size_t)n * 8));
    TRY(c->wh_order.reserve((size_t)s.N * 4));
    TRY(c->wh_ws.reserve(bucket_sort_workspace_bytes(s.N, M)));
    double *hd = c->hist.as<double>();
    TRY(launch_bucket_sort(idx, s.N, M, c->wh_order.as<int32_t>(), c->wh_ws.p, c->stream));
    TRY(dbgsom_class_histogram_weighted(c->wh_order.as<int32_t>(), bucket_sort_seg_start(c->wh_ws.p, s.N, M), c->y.as<int32_t>(),
                                        c->sw.as<double>(), s.N, M, n_classes, hd, c->stream));
    TRY(run_allreduce(c, hd, n));
    DBGSOM_HIP_CHECK(hipMemcpyAsync(hist_host, hd, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    return sync(c);
}

// ------------------------------------------------------------------------------------------
// per-unit sums of a per-row quantity, and the statistics of attached targets: csrc/unit_sums.hip
// ------------------------------------------------------------------------------------------
namespace {

int unit_args_check(const char *fn, bool pointers, int64_t N, int64_t M, int n_values, int64_t ld_in, int64_t ld_out) {
    const char *why = nullptr;
    if (!pointers) why = "null pointer";
    else if (N < 0 || N > 0x7fffffffLL) why = "N must be 0 .. 2^31 - 1";
    else if (M < 1 || M > DBGSOM_MAX_PROTOTYPES) why = "M must be 1 .. DBGSOM_MAX_PROTOTYPES";
    else if (n_values < 1 || n_values > DBGSOM_MAX_MIXTURE_VALUES) why = "n_values must be 1 .. DBGSOM_MAX_MIXTURE_VALUES";
    else if (ld_in < n_values) why = "a row stride of the input is below n_values";
    else if (ld_out < n_values) why = "a row stride of the output is below n_values";
    if (why) { set_error("%s: %s", fn, why); return DBGSOM_EINVAL; }
    return DBGSOM_OK;
}

// the fold on device buffers, on the context's stream, not waited for
int unit_sums_launch(dbgsom_ctx *c, const int64_t *unit, const double *Z, int64_t ldz, const double *w, int64_t N, int64_t M,
                     int V, double *mass, double *sums, int64_t lds) {
    TRY(c->us_ws.reserve(unit_sums_workspace_bytes(N, M, V, w != nullptr)));
    return launch_unit_sums(unit, Z, ldz, w, N, M, V, mass, sums, lds, c->us_ws.p, c->us_ws.cap, c->stream);
}

// out[j, v] = num[j, v] / mass[j], or its square root: one division (and one root) per entry
__global__ __launch_bounds__(256) void unit_ratio_kernel(const double *num, const double *__restrict__ mass, int64_t M,
                                                         int V, int root, double *out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= M * V) return;
    const double q = num[e] / mass[e / V];
    out[e] = root ? __dsqrt_rn(q) : q;
}

}  // namespace

int dbgsom_ctx_unit_sums(dbgsom_ctx *c, const int64_t *unit_host, const double *Z_host, const double *w_host, int64_t N,
                         int64_t M, int n_values, double *mass_host, double *sums_host) {
    TRY(unit_args_check(__func__, mass_host && sums_host && (N == 0 || (unit_host && Z_host)), N, M, n_values, n_values,
                        n_values));
    CTX_CHECK(c);
    const int V = n_values;
    const size_t bu = align_up((size_t)N * 8), bz = align_up((size_t)N * V * 8), bw = w_host ? bu : 0;
    TRY(c->us_in.reserve(bu + bz + bw + 256));
    TRY(c->us_out.reserve(align_up((size_t)M * (V + 1) * 8)));
    char *base = c->us_in.as<char>();
    int64_t *unit = reinterpret_cast<int64_t *>(base);
    double *Z = reinterpret_cast<double *>(base + bu);
    double *w = w_host ? reinterpret_cast<double *>(base + bu + bz) : nullptr;
    if (N) {
        DBGSOM_HIP_CHECK(hipMemcpyAsync(unit, unit_host, (size_t)N * 8, hipMemcpyHostToDevice, c->stream));
        DBGSOM_HIP_CHECK(hipMemcpyAsync(Z, Z_host, (size_t)N * V * 8, hipMemcpyHostToDevice, c->stream));
        if (w) DBGSOM_HIP_CHECK(hipMemcpyAsync(w, w_host, (size_t)N * 8, hipMemcpyHostToDevice, c->stream));
        c->x_up((size_t)N * 8 * (1 + V + (w ? 1 : 0)));
    }
    double *mass = c->us_out.as<double>(), *sums = mass + M;
    int rc = unit_sums_launch(c, unit, Z, V, w, N, M, V, mass, sums, V);
    if (rc == DBGSOM_OK) {
        DBGSOM_HIP_CHECK(hipMemcpyAsync(mass_host, mass, (size_t)M * 8, hipMemcpyDeviceToHost, c->stream));
        DBGSOM_HIP_CHECK(hipMemcpyAsync(sums_host, sums, (size_t)M * V * 8, hipMemcpyDeviceToHost, c->stream));
        c->x_down((size_t)M * (V + 1) * 8);
    }
    return finish_query(c, rc);
}

int dbgsom_ctx_unit_sums_device(dbgsom_ctx *c, const int64_t *unit_dev, const double *Z_dev, int64_t ldz, const double *w_dev,
                                int64_t N, int64_t M, int n_values, double *mass_dev, double *sums_dev, int64_t lds) {
    TRY(unit_args_check(__func__, mass_dev && sums_dev && (N == 0 || (unit_dev && Z_dev)), N, M, n_values, ldz, lds));
    CTX_CHECK(c);
    return finish_query(c, unit_sums_launch(c, unit_dev, Z_dev, ldz, w_dev, N, M, n_values, mass_dev, sums_dev, lds));
}

int dbgsom_ctx_unit_deviations_device(dbgsom_ctx *c, const int64_t *unit_dev, const double *Y_dev, int64_t ldy, int64_t N,
                                      const double *C_dev, int64_t ldc, int64_t M, int n_values, int mode, double *out_dev,
                                      int64_t ldo) {
    DBGSOM_REQUIRE(mode == DBGSOM_DEVIATIONS_SQUARES || mode == DBGSOM_DEVIATIONS_NORM,
                   "mode must be DBGSOM_DEVIATIONS_SQUARES or DBGSOM_DEVIATIONS_NORM");
    TRY(unit_args_check(__func__, N == 0 || (unit_dev && Y_dev && C_dev && out_dev), N, M, n_values, ldy < ldc ? ldy : ldc,
                        mode == DBGSOM_DEVIATIONS_SQUARES ? ldo : n_values));
    CTX_CHECK(c);
    return finish_query(c, launch_unit_deviations(unit_dev, Y_dev, ldy, N, C_dev, ldc, M, n_values, mode, out_dev, ldo,
                                                  c->stream));
}

int dbgsom_ctx_set_targets(dbgsom_ctx *c, const double *Y_host, int64_t N, int n_values) {
    if (!Y_host) {
        CTX_CHECK(c);
        c->has_targets = false;
        return DBGSOM_OK;
    }
    DBGSOM_REQUIRE(n_values >= 1 && n_values <= DBGSOM_MAX_MIXTURE_VALUES, "n_values must be 1 .. DBGSOM_MAX_MIXTURE_VALUES");
    CTX_CHECK(c);
    TRY(loaded(c, __func__));
    DBGSOM_REQUIRE(N == c->xs.N, "one row of targets per resident sample");
    c->has_targets = false;
    TRY(c->ty.reserve((size_t)N * n_values * 8));
    DBGSOM_HIP_CHECK(hipMemcpyAsync(c->ty.p, Y_host, (size_t)N * n_values * 8, hipMemcpyHostToDevice, c->stream));
    c->x_up((size_t)N * n_values * 8);
    c->target_V = n_values;
    c->has_targets = true;
    return sync(c);
}

int dbgsom_ctx_set_targets_device(dbgsom_ctx *c, const double *Y_dev, int64_t N, int64_t ldy, int n_values) {
    DBGSOM_REQUIRE(Y_dev, "null pointer");
    DBGSOM_REQUIRE(n_values >= 1 && n_values <= DBGSOM_MAX_MIXTURE_VALUES, "n_values must be 1 .. DBGSOM_MAX_MIXTURE_VALUES");
    DBGSOM_REQUIRE(ldy >= n_values, "ldy below n_values");
    CTX_CHECK(c);
    TRY(loaded(c, __func__));
    DBGSOM_REQUIRE(N == c->xs.N, "one row of targets per resident sample");
    c->has_targets = false;
    TRY(c->ty.reserve((size_t)N * n_values * 8));
    DBGSOM_HIP_CHECK(hipMemcpy2DAsync(c->ty.p, (size_t)n_values * 8, Y_dev, (size_t)ldy * 8, (size_t)n_values * 8, (size_t)N,
                                      hipMemcpyDeviceToDevice, c->stream));
    c->target_V = n_values;
    c->has_targets = true;
    return sync(c);
}

int dbgsom_ctx_target_statistics(dbgsom_ctx *c, const int64_t *idx_host, int64_t M, double *mass_host, double *mean_host,
                                 double *std_host, double *err_host) {
    DBGSOM_REQUIRE(mass_host && mean_host, "null pointer");
    DBGSOM_REQUIRE(M >= 1 && M <= DBGSOM_MAX_PROTOTYPES, "M must be 1 .. DBGSOM_MAX_PROTOTYPES");
    CTX_CHECK(c);
    TRY(loaded(c, __func__));
    DBGSOM_REQUIRE(c->coll_nranks == 1 && !c->allreduce, "more than one rank");
    if (!c->has_targets) { set_error("target statistics requested but no targets attached (dbgsom_ctx_set_targets)"); return DBGSOM_ESTATE; }
    Samples &s = c->xs;
    const int64_t N = s.N;
    const int V = c->target_V;
    const int64_t *idx = nullptr;
    if (idx_host) {
        TRY(c->qidx.reserve((size_t)N * 8));
        DBGSOM_HIP_CHECK(hipMemcpyAsync(c->qidx.p, idx_host, (size_t)N * 8, hipMemcpyHostToDevice, c->stream));
        idx = c->qidx.as<int64_t>();
    } else {
        if (!c->search.last_idx_valid) { set_error("no winners of a previous epoch in HBM"); return DBGSOM_ESTATE; }
        idx = c->idx[c->icur].as<int64_t>();
    }
    // [mass | sums | mean | mass of the second fold | squares / std | err]
    const size_t mv = (size_t)M * V;
    TRY(c->us_out.reserve((3 * mv + 3 * (size_t)M) * 8));
    if (std_host || err_host) TRY(c->us_dev.reserve((size_t)N * V * 8));
    double *mass = c->us_out.as<double>(), *sums = mass + M, *mean = sums + mv, *mass2 = mean + mv, *sq = mass2 + M,
           *err = sq + mv;
    const double *Y = c->ty.as<double>(), *w = c->has_weights ? c->sw.as<double>() : nullptr;
    double *dev = c->us_dev.as<double>();
    TRY(unit_sums_launch(c, idx, Y, V, w, N, M, V, mass, sums, V));
    hipLaunchKernelGGL(unit_ratio_kernel, dim3(grid1d((int64_t)mv)), dim3(256), 0, c->stream, (const double *)sums,
                       (const double *)mass, M, V, 0, mean);
    TRY(launch_status("unit_ratio_kernel"));
    DBGSOM_HIP_CHECK(hipMemcpyAsync(mass_host, mass, (size_t)M * 8, hipMemcpyDeviceToHost, c->stream));
    DBGSOM_HIP_CHECK(hipMemcpyAsync(mean_host, mean, mv * 8, hipMemcpyDeviceToHost, c->stream));
    if (std_host) {
        TRY(launch_unit_deviations(idx, Y, V, N, mean, V, M, V, DBGSOM_DEVIATIONS_SQUARES, dev, V, c->stream));
        TRY(unit_sums_launch(c, idx, dev, V, w, N, M, V, mass2, sq, V));
        hipLaunchKernelGGL(unit_ratio_kernel, dim3(grid1d((int64_t)mv)), dim3(256), 0, c->stream, (const double *)sq,
                           (const double *)mass2, M, V, 1, sq);
        TRY(launch_status("unit_ratio_kernel"));
        DBGSOM_HIP_CHECK(hipMemcpyAsync(std_host, sq, mv * 8, hipMemcpyDeviceToHost, c->stream));
    }
    if (err_host) {
        TRY(launch_unit_deviations(idx, Y, V, N, mean, V, M, V, DBGSOM_DEVIATIONS_NORM, dev, 1, c->stream));
        TRY(unit_sums_launch(c, idx, dev, 1, w, N, M, 1, mass2, err, 1));
        DBGSOM_HIP_CHECK(hipMemcpyAsync(err_host, err, (size_t)M * 8, hipMemcpyDeviceToHost, c->stream));
    }
    return sync(c);
}

// ------------------------------------------------------------------------------------------
// vertical growth
// ------------------------------------------------------------------------------------------
int dbgsom_ctx_partition(dbgsom_ctx *c, const double *W_host, int64_t M, int round_f32, int64_t *counts_host,
                         int64_t *idx_host) {
    CTX_CHECK(c);
    TRY(loaded(c, __func__));
    TRY(complete_rows(c, __func__));
    DBGSOM_REQUIRE(counts_host && M >= 1 && M <= DBGSOM_MAX_PROTOTYPES, "bad arguments");
    Samples &s = c->xs;
    TRY(resident_bmu(c, W_host, M, 1, round_f32));
    TRY(c->part_order.reserve((size_t)s.N * 4));
    TRY(c->part_ws.reserve(bucket_sort_workspace_bytes(s.N, M)));
    TRY(c->part_counts.reserve((size_t)(M + 1) * 8));
    TRY(launch_bucket_sort(c->qidx.as<int64_t>(), s.N, M, c->part_order.as<int32_t>(), c->part_ws.p, c->stream));
    const uint32_t *seg_start = bucket_sort_seg_start(c->part_ws.p, s.N, M);
    hipLaunchKernelGGL(seg_counts_kernel, dim3(grid1d(M)), dim3(256), 0, c->stream, seg_start, M, s.N, c->part_counts.as<int64_t>());
    TRY(launch_status("seg_counts_kernel"));
    DBGSOM_HIP_CHECK(hipMemcpyAsync(counts_host, c->part_counts.p, (size_t)M * 8, hipMemcpyDeviceToHost, c->stream));
    if (idx_host) DBGSOM_HIP_CHECK(hipMemcpyAsync(idx_host, c->qidx.p, (size_t)s.N * 8, hipMemcpyDeviceToHost, c->stream));
    TRY(sync(c));
    c->partM = M;
    c->part_valid = true;
    return DBGSOM_OK;
}

int dbgsom_ctx_read_partition(dbgsom_ctx *c, int32_t *order_host, uint32_t *seg_start_host) {
    CTX_CHECK(c);
    TRY(loaded(c, __func__));
    if (!c->part_valid) { set_error("dbgsom_ctx_read_partition: call dbgsom_ctx_partition first"); return DBGSOM_ESTATE; }
    const Samples &s = c->xs;
    if (order_host)
        DBGSOM_HIP_CHECK(hipMemcpyAsync(order_host, c->part_order.p, (size_t)s.N * 4, hipMemcpyDeviceToHost, c->stream));
    if (seg_start_host)
        DBGSOM_HIP_CHECK(hipMemcpyAsync(seg_start_host, bucket_sort_seg_start(c->part_ws.p, s.N, c->partM),
                                        (size_t)(c->partM + 1) * 4, hipMemcpyDeviceToHost, c->stream));
    return sync(c);
}

int dbgsom_ctx_subset_create(dbgsom_ctx *c, int64_t neuron, dbgsom_ctx **child_out) {
    CTX_CHECK(c);
    TRY(loaded(c, __func__));
    TRY(complete_rows(c, __func__));
    DBGSOM_REQUIRE(child_out, "null pointer");
    *child_out = nullptr;
    if (c->xs.csr) { set_error("dbgsom_ctx_subset_create: the resident samples are CSR (select the rows on the host and load them)"); return DBGSOM_ESTATE; }
    if (!c->part_valid) { set_error("dbgsom_ctx_subset_create: call dbgsom_ctx_partition first"); return DBGSOM_ESTATE; }
    DBGSOM_REQUIRE(neuron >= 0 && neuron < c->partM, "neuron out of range");
    Samples &s = c->xs;
    const uint32_t *seg_start = bucket_sort_seg_start(c->part_ws.p, s.N, c->partM);
    uint32_t seg[2] = {0, 0};
    DBGSOM_HIP_CHECK(hipMemcpyAsync(&seg[0], seg_start + neuron, 4, hipMemcpyDeviceToHost, c->stream));
    if (neuron + 1 < c->partM)
        DBGSOM_HIP_CHECK(hipMemcpyAsync(&seg[1], seg_start + neuron + 1, 4, hipMemcpyDeviceToHost, c->stream));
    TRY(sync(c));
    if (neuron + 1 >= c->partM) seg[1] = (uint32_t)s.N;
    const int64_t first = seg[0], n = (int64_t)seg[1] - (int64_t)seg[0];
    if (n < 1) { set_error("dbgsom_ctx_subset_create: neuron %lld has no samples", (long long)neuron); return DBGSOM_EINVAL; }
    dbgsom_ctx *k = nullptr;
    TRY(dbgsom_ctx_create(c->device, &k));
    k->policy.algorithm = c->policy.algorithm; k->policy.sweep_planes = c->policy.sweep_planes;
    k->policy.seed_stride = c->policy.seed_stride; k->policy.max_mean_candidates = c->policy.max_mean_candidates;
    k->filter_min_query_rows = c->filter_min_query_rows;
    k->allreduce = nullptr;  // a child map is fitted on this rank's rows alone
    Samples &t = k->xs;
    int rc = DBGSOM_OK;
    do {
        const size_t es = dtype_size(s.dtype);
        if ((rc = t.own.reserve((size_t)n * s.dp * es))) break;
        t.N = n; t.d = s.d; t.dp = s.dp; t.dtype = s.dtype; t.X = t.own.p;
        const int32_t *order = c->part_order.as<int32_t>();
        // the gather runs on the parent's stream (it reads the parent's buffers), then both are idle
        if (s.dtype == DBGSOM_F32)
            hipLaunchKernelGGL(gather_rows_kernel<float>, dim3((unsigned)n), dim3(256), 0, c->stream, (const float *)s.X, s.dp, order, first, n, s.dp, (float *)t.own.p);
        else if (s.dtype == DBGSOM_F64)
            hipLaunchKernelGGL(gather_rows_kernel<double>, dim3((unsigned)n), dim3(256), 0, c->stream, (const double *)s.X, s.dp, order, first, n, s.dp, (double *)t.own.p);
        else
            hipLaunchKernelGGL(gather_rows_kernel<uint16_t>, dim3((unsigned)n), dim3(256), 0, c->stream, (const uint16_t *)s.X, s.dp, order, first, n, s.dp, (uint16_t *)t.own.p);
        if ((rc = launch_status("gather_rows_kernel"))) break;
        if (c->has_labels) {
            if ((rc = k->y.reserve((size_t)n * 4))) break;
            hipLaunchKernelGGL(gather_i32_kernel, dim3(grid1d(n)), dim3(256), 0, c->stream, c->y.as<int32_t>(), order, first, n, k->y.as<int32_t>());
            if ((rc = launch_status("gather_i32_kernel"))) break;
            k->has_labels = true;
        }
        if (c->has_weights) {
            if ((rc = k->sw.reserve((size_t)n * 8))) break;
            hipLaunchKernelGGL(gather_f64_kernel, dim3(grid1d(n)), dim3(256), 0, c->stream, c->sw.as<double>(), order, first, n, k->sw.as<double>());
            if ((rc = launch_status("gather_f64_kernel"))) break;
            k->has_weights = true;
        }
        if ((rc = sync(c))) break;
        if ((rc = finish_samples(k, t, false))) break;
        rc = sync(k);
    } while (0);
    if (rc != DBGSOM_OK) { (void)hipStreamSynchronize(c->stream); dbgsom_ctx_destroy(k); return rc; }
    *child_out = k;
    return DBGSOM_OK;
}

// ------------------------------------------------------------------------------------------
// diagnostics
// ------------------------------------------------------------------------------------------
int dbgsom_ctx_epoch_info(dbgsom_ctx *c, double *info8) {
    CTX_CHECK(c);
    DBGSOM_REQUIRE(info8, "null pointer");
    info8[0] = c->last_filtered ? 1.0 : 0.0;
    const SearchPolicy &pol = c->policy;
    info8[1] = pol.last_mean;
    info8[2] = c->last_filtered ? (double)pol.planes_used : 0.0;
    info8[3] = pol.last_hinted ? 1.0 : 0.0;
    info8[4] = (double)pol.filter_backoff;
    info8[5] = (double)pol.plane_hold;
    info8[6] = c->last_filtered && pol.last_probed ? pol.last_probe_mean : NAN;
    info8[7] = c->last_filtered && pol.last_seed_full ? 1.0 : 0.0;
    return DBGSOM_OK;
}

int dbgsom_ctx_arm_ms(dbgsom_ctx *c, double *ms12) {
    CTX_CHECK(c);
    DBGSOM_REQUIRE(ms12, "null pointer");
    for (int s_ = 0; s_ < 3; ++s_)
        for (int q = 0; q < 4; ++q) ms12[4 * s_ + q] = c->policy.arm_ms[s_][q];
    return DBGSOM_OK;
}

int dbgsom_ctx_filter_counts(dbgsom_ctx *c, uint32_t *counts_host, int64_t n) {
    CTX_CHECK(c);
    DBGSOM_REQUIRE(counts_host, "null pointer");
    if (!c->last_filter_ws) { set_error("dbgsom_ctx_filter_counts: no filtered search has run"); return DBGSOM_ESTATE; }
    return dbgsom_bmu_filtered_counts(c->last_filter_ws, c->last_filter_N, c->last_filter_d, c->last_filter_M, counts_host, n,
                                      c->stream);
}

int dbgsom_ctx_refine_counts(dbgsom_ctx *c, uint64_t *out4) {
    CTX_CHECK(c);
    DBGSOM_REQUIRE(out4, "null pointer");
    if (!c->last_filter_ws) { set_error("dbgsom_ctx_refine_counts: no filtered search has run"); return DBGSOM_ESTATE; }
    return dbgsom_bmu_filtered_refine_counts(c->last_filter_ws, c->last_filter_N, c->last_filter_d, c->last_filter_M, out4,
                                             c->stream);
}

int dbgsom_ctx_read_anchors(dbgsom_ctx *c, int64_t *n_anchors, double *anchors_host, int32_t *anchor_of_host,
                            int32_t *order_host, int32_t *aseed_host) {
    CTX_CHECK(c);
    TRY(loaded(c, __func__));
    TRY(complete_rows(c, __func__));
    Samples &s = c->xs;
    if (s.anchor_state != 1) { set_error("dbgsom_ctx_read_anchors: the resident samples have no anchor buckets"); return DBGSOM_ESTATE; }
    if (aseed_host && !(c->anchor.last_anchor_seeded && c->last_filter_ws)) {
        set_error("dbgsom_ctx_read_anchors: the last search was not seeded from the anchors");
        return DBGSOM_ESTATE;
    }
    const int64_t A = s.n_anchors;
    if (n_anchors) *n_anchors = A;
    if (anchors_host)
        DBGSOM_HIP_CHECK(hipMemcpyAsync(anchors_host, s.anchors.p, (size_t)A * s.dp * 8, hipMemcpyDeviceToHost, c->stream));
    if (anchor_of_host)
        DBGSOM_HIP_CHECK(hipMemcpyAsync(anchor_of_host, s.anchor_of.p, (size_t)s.N * 4, hipMemcpyDeviceToHost, c->stream));
    if (order_host)
        DBGSOM_HIP_CHECK(hipMemcpyAsync(order_host, s.anchor_order.p, (size_t)s.N * 4, hipMemcpyDeviceToHost, c->stream));
    if (aseed_host)
        return dbgsom_bmu_filtered_anchor_seeds(c->last_filter_ws, c->last_filter_N, c->last_filter_d, c->last_filter_M, (int)A,
                                                aseed_host, nullptr, c->stream);
    return sync(c);
}

int dbgsom_ctx_read_anchor_runs(dbgsom_ctx *c, int64_t *n_groups, int32_t *run_start_host, int32_t *run_anchor_host,
                                double *run_R_host, double *run_xx_host) {
    CTX_CHECK(c);
    TRY(loaded(c, __func__));
    TRY(complete_rows(c, __func__));
    Samples &s = c->xs;
    if (s.anchor_state != 1) { set_error("dbgsom_ctx_read_anchor_runs: the resident samples have no anchor buckets"); return DBGSOM_ESTATE; }
    if (n_groups) *n_groups = (s.N + 127) / 128;
    if (!run_start_host) return DBGSOM_OK;
    return dbgsom_anchor_runs_read(s.anchor_runs.p, s.N, (int)s.n_anchors, run_start_host, run_anchor_host, run_R_host,
                                   run_xx_host, c->stream);
}

int dbgsom_ctx_phase_ms(dbgsom_ctx *c, double *ms8) {
    CTX_CHECK(c);
    DBGSOM_REQUIRE(ms8, "null pointer");
    if (!c->timing || !c->ev_valid) { set_error("dbgsom_ctx_phase_ms: no timed epoch (set option \"timing\")"); return DBGSOM_ESTATE; }
    for (int k = 0; k < 3; ++k) {
        float ms = 0.f;
        DBGSOM_HIP_CHECK(hipEventElapsedTime(&ms, c->ev[k], c->ev[k + 1]));
        ms8[k] = ms;
    }
    for (int k = 0; k < 5; ++k) ms8[3 + k] = c->filter_ms_valid ? c->filter_ms[k] : 0.0;
    return DBGSOM_OK;
}

}  // extern "C"
