// Fit on rows with missing entries (NaN) on gfx950: the per-(neuron, feature) sums of one epoch.
//
// Per neuron j and feature c, over the rows i with win_i = j whose entry c is observed (x_ic == x_ic):
//   S_jc = sum kw_i x_ic     K_jc = sum kw_i     A_jc = their number
// and per neuron over all of its rows: a_j = their number, E_j = sum dist_i.  Layout of `sums` (float64,
// M (3 d + 2) values, every part a sum over rows and therefore all-reducible): [S (M x d) | K (M x d) | A (M x d) | a | E].
//
// A sibling of segsum_kernel (accumulate.hip) and built the same way: the rows are bucketed by winner with the
// stable counting sort (launch_bucket_sort), every neuron's list is cut into chunks of <= CH rows, one workgroup
// sums one chunk in list order into a slab row (3 d + 2 wide), and a second pass adds a neuron's chunk partials in
// chunk order (small maps: in NG groups side by side, then in group order).  No floating-point atomics; the
// result depends on the winners alone, not on the grid.  X is streamed once, 16 bytes per lane past the caches.
// Per column a lane keeps three accumulators and the test v == v decides whether kw v, kw and 1 are added: an
// unobserved entry adds nothing, so a (neuron, feature) nobody observed keeps exact zeros in all three.
// Only the first d columns of a row are data: what sits behind them (the zero padding of resident rows, junk
// or NaN of a raw caller) is loaded with the last 16-byte piece at most and never added or stored.
#include "common.h"

namespace dbgsom {

constexpr int FT = 256;    // threads per workgroup
constexpr int FCH = 128;   // rows per chunk: accumulate.hip's CH (the bucket sort cuts chunk_pre by it; checked at launch)

// (the 16-byte non-temporal row loads of segsum_kernel)
template <typename XT, int VEC>
__device__ __forceinline__ void load_piece(const XT *__restrict__ src, XT (&v)[VEC]) {
    if constexpr (sizeof(XT) == 4 && VEC == 4) {
        typedef float f4_t __attribute__((ext_vector_type(4)));
        const f4_t t4 = __builtin_nontemporal_load(reinterpret_cast<const f4_t *>(src));
        v[0] = t4.x; v[1] = t4.y; v[2] = t4.z; v[3] = t4.w;
    } else if constexpr (sizeof(XT) == 8 && VEC == 2) {
        typedef double d2_t __attribute__((ext_vector_type(2)));
        const d2_t t2 = __builtin_nontemporal_load(reinterpret_cast<const d2_t *>(src));
        v[0] = t2.x; v[1] = t2.y;
    } else {
        static_assert(VEC == 1, "unsupported vector width");
        v[0] = src[0];
    }
}

// ---- a winner outside [0, M): the status flag (the sort itself skips such rows) -------------------------------
__global__ __launch_bounds__(FT) void winner_range_kernel(const int64_t *__restrict__ win, int64_t N, int64_t M,
                                                          int32_t *__restrict__ status) {
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * FT + threadIdx.x; i < N; i += (int64_t)gridDim.x * FT) {
        const int64_t j = win[i];
        bad |= (j < 0 || j >= M);
    }
    if (bad) atomicOr(status, 1);
}

// ---- one workgroup sums one chunk (<= FCH rows of one neuron) in list order ------------------------------------
// slab row: [S (d) | K (d) | A (d) | rows of the chunk | sum of their distances]
template <typename XT, int VEC>
__global__ __launch_bounds__(FT) void segsum_masked_kernel(
    const XT *__restrict__ X, int d, int64_t ldx, const int32_t *__restrict__ order, const double *__restrict__ kw,
    const double *__restrict__ dist, const uint32_t *__restrict__ seg_start, const uint32_t *__restrict__ count,
    const uint32_t *__restrict__ chunk_pre, int M, double *__restrict__ slab) {
    __shared__ int32_t rows_s[FCH];
    __shared__ double kw_s[FCH];
    __shared__ double dist_s[FCH];
    __shared__ double red[3 * FT * VEC];
    __shared__ uint32_t info[2];
    const int tid = threadIdx.x;
    const uint32_t c = blockIdx.x;
    if (c >= chunk_pre[M]) return;  // uniform per workgroup
    if (tid == 0) {
        int lo = 0, hi = M;  // last j with chunk_pre[j] <= c
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (chunk_pre[mid] <= c) lo = mid; else hi = mid;
        }
        const uint32_t begin = seg_start[lo] + (c - chunk_pre[lo]) * FCH;
        const uint32_t end = min(begin + (uint32_t)FCH, seg_start[lo] + count[lo]);
        info[0] = begin; info[1] = end - begin;
    }
    __syncthreads();
    const uint32_t begin = info[0];
    const int n = (int)info[1];
    if (tid < n) {
        const int32_t r = order[begin + tid];
        rows_s[tid] = r;
        kw_s[tid] = kw[r];
        dist_s[tid] = dist[r];
    }
    __syncthreads();
    double *out = slab + (size_t)c * (3 * (size_t)d + 2);
    if (tid == FT - 1) {  // the scalar partials, in list order
        double se = 0.0;
        for (int p = 0; p < n; ++p) se += dist_s[p];
        out[3 * (size_t)d] = (double)n;
        out[3 * (size_t)d + 1] = se;
    }
    const int Q = (d + VEC - 1) / VEC;  // column groups; the last one may reach behind column d
    // the rows p0, p0 + step, ... of the chunk on column group q
    auto walk = [&](int q, int p0, int step, double (&aS)[VEC], double (&aK)[VEC], double (&aA)[VEC]) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) aS[e] = aK[e] = aA[e] = 0.0;
#pragma unroll 4
        for (int p = p0; p < n; p += step) {
            const XT *src = X + (int64_t)rows_s[p] * ldx + (int64_t)q * VEC;
            const double w = kw_s[p];
            XT v[VEC];
            load_piece<XT, VEC>(src, v);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                if (v[e] == v[e]) {   // observed
                    aS[e] += w * widen(v[e]);
                    aK[e] += w;
                    aA[e] += 1.0;
                }
            }
        }
    };
    if (Q >= FT) {
        for (int q = tid; q < Q; q += FT) {
            double aS[VEC], aK[VEC], aA[VEC];
            walk(q, 0, 1, aS, aK, aA);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const int col = q * VEC + e;
                if (col < d) { out[col] = aS[e]; out[(size_t)d + col] = aK[e]; out[2 * (size_t)d + col] = aA[e]; }
            }
        }
    } else {
        const int RL = FT / Q;  // row lanes working side by side on the same column group
        const int rl = tid / Q, q = tid - rl * Q;
        if (rl < RL) {
            double aS[VEC], aK[VEC], aA[VEC];
            walk(q, rl, RL, aS, aK, aA);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                red[(0 * FT + rl * Q + q) * VEC + e] = aS[e];
                red[(1 * FT + rl * Q + q) * VEC + e] = aK[e];
                red[(2 * FT + rl * Q + q) * VEC + e] = aA[e];
            }
        }
        __syncthreads();
        if (rl == 0) {  // row lanes are added in lane order
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const int col = q * VEC + e;
                if (col >= d) continue;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    double s = red[(a * FT + q) * VEC + e];
                    for (int u = 1; u < RL; ++u) s += red[(a * FT + u * Q + q) * VEC + e];
                    out[(size_t)a * d + col] = s;
                }
            }
        }
    }
}

// ---- add each neuron's chunk partials in chunk order -----------------------------------------------------------
// where column `col` of neuron j's slab row goes in [S | K | A | a | E]
__device__ __forceinline__ void store_masked_sum(double *__restrict__ sums, int64_t M, int64_t d, int64_t j, int64_t col,
                                                 double s) {
    if (col < 3 * d) {
        const int64_t plane = col / d;
        sums[plane * M * d + j * d + (col - plane * d)] = s;
    } else {
        sums[3 * M * d + (col - 3 * d) * M + j] = s;   // a (an exact integer: the sum of the chunks' row counts), then E
    }
}

__global__ __launch_bounds__(FT) void finalize_masked_kernel(const double *__restrict__ slab, int d, int M,
                                                             const uint32_t *__restrict__ chunk_pre, int NG,
                                                             double *__restrict__ gslab, double *__restrict__ sums) {
    const int j = blockIdx.x, g = blockIdx.y;
    const int64_t W3 = 3 * (int64_t)d + 2;
    const uint32_t b0 = chunk_pre[j], b1 = chunk_pre[j + 1];
    const uint32_t per = (b1 - b0 + NG - 1) / NG;  // chunks per group
    const uint32_t c0 = min(b1, b0 + g * per), c1 = min(b1, c0 + per);
    for (int64_t col = threadIdx.x + FT * blockIdx.z; col < W3; col += (int64_t)FT * gridDim.z) {
        double s = 0.0;
        uint32_t c = c0;
        for (; c + 8 <= c1; c += 8) {  // loads batched, additions still in chunk order
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = slab[(size_t)(c + u) * W3 + col];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
        for (; c < c1; ++c) s += slab[(size_t)c * W3 + col];
        if (NG > 1) gslab[((size_t)j * NG + g) * W3 + col] = s;
        else store_masked_sum(sums, M, d, j, col, s);
    }
}

// second level (NG > 1): the NG group sums of a neuron in group order
__global__ __launch_bounds__(FT) void finalize_masked_groups_kernel(const double *__restrict__ gslab, int d, int M, int NG,
                                                                    double *__restrict__ sums) {
    const int j = blockIdx.x;
    const int64_t W3 = 3 * (int64_t)d + 2;
    for (int64_t col = threadIdx.x + FT * blockIdx.y; col < W3; col += (int64_t)FT * gridDim.y) {
        double s = 0.0;
        for (int g = 0; g < NG; ++g) s += gslab[((size_t)j * NG + g) * W3 + col];
        store_masked_sum(sums, M, d, j, col, s);
    }
}

// -------------------------------------------------------------------------------------------------------------
// (a small map has few neurons with very many chunk partials each: accumulate.hip's grouping, a function of M alone)
static int masked_groups(int64_t M) {
    const int64_t g = 512 / (M > 0 ? M : 1);
    return (int)(g < 1 ? 1 : (g > 32 ? 32 : g));
}

struct MaskedAccWs {
    int32_t *order;   // N        sample ids, bucketed by winner, stable
    void *sort_ws;    //          launch_bucket_sort's tables (count, seg_start, chunk_pre among them)
    double *slab;     // maxchunks x (3 d + 2)
    double *gslab;    // M x NG x (3 d + 2)
    int64_t maxchunks;
};

static size_t carve_masked(MaskedAccWs *w, char *base, int64_t N, int64_t d, int64_t M) {
    const int64_t maxchunks = (N + FCH - 1) / FCH + M;
    const size_t W3 = 3 * (size_t)d + 2;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += align_up(bytes); return o; };
    const size_t o_order = take((size_t)N * 4);
    const size_t o_sort = take(bucket_sort_workspace_bytes(N, M));
    const size_t o_slab = take((size_t)maxchunks * W3 * 8);
    const size_t o_gslab = take((size_t)M * masked_groups(M) * W3 * 8);
    if (w) {
        w->order = (int32_t *)(base + o_order);
        w->sort_ws = base + o_sort;
        w->slab = (double *)(base + o_slab);
        w->gslab = (double *)(base + o_gslab);
        w->maxchunks = maxchunks;
    }
    return off;
}

static bool masked_acc_shape_ok(int64_t N, int64_t d, int64_t M) {
    return N >= 0 && N < 0x7fffffff && d >= 1 && d <= 0x0fffffff && M >= 1 && M <= DBGSOM_MAX_PROTOTYPES;
}

size_t accumulate_masked_workspace_bytes(int64_t N, int64_t d, int64_t M) {
    if (!masked_acc_shape_ok(N, d, M)) return 0;
    return carve_masked(nullptr, nullptr, N, d, M);
}

int launch_accumulate_masked(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const int64_t *idx,
                             const double *kw, const double *dist, int64_t M, double *sums, int32_t *status, void *ws,
                             size_t ws_bytes, hipStream_t s) {
    DBGSOM_REQUIRE(x_dtype == DBGSOM_F32 || x_dtype == DBGSOM_F64, "x_dtype must be DBGSOM_F32 or DBGSOM_F64");
    DBGSOM_REQUIRE(N >= 0 && N < 0x7fffffff && d >= 1 && d <= 0x0fffffff && ldx >= d, "bad sample shape");
    DBGSOM_REQUIRE(M >= 1 && M <= DBGSOM_MAX_PROTOTYPES, "M outside [1, DBGSOM_MAX_PROTOTYPES]");
    DBGSOM_REQUIRE(sums, "null sums");
    DBGSOM_REQUIRE(accumulate_chunk_rows() == FCH, "chunk length differs from the bucket sort's");
    const size_t n_sums = (size_t)M * (3 * (size_t)d + 2);
    if (N == 0) {
        if (status) DBGSOM_HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int32_t), s));
        DBGSOM_HIP_CHECK(hipMemsetAsync(sums, 0, n_sums * sizeof(double), s));
        return DBGSOM_OK;
    }
    DBGSOM_REQUIRE(X && idx && kw && dist && ws, "null pointer");
    DBGSOM_REQUIRE(is_aligned(ws, 256), "workspace must be 256-byte aligned");
    const size_t need = accumulate_masked_workspace_bytes(N, d, M);
    if (ws_bytes < need) {
        set_error("dbgsom_accumulate_masked: workspace too small (%zu < %zu)", ws_bytes, need);
        return DBGSOM_ENOMEM;
    }
    MaskedAccWs w;
    carve_masked(&w, (char *)ws, N, d, M);
    const int Mi = (int)M, di = (int)d;
    if (status) {
        DBGSOM_HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int32_t), s));
        const int64_t nb = (N + FT - 1) / FT;
        hipLaunchKernelGGL(winner_range_kernel, dim3((unsigned)(nb > 2048 ? 2048 : nb)), dim3(FT), 0, s, idx, N, M, status);
    }
    TRY_STATUS(launch_bucket_sort(idx, N, M, w.order, w.sort_ws, s));
    const uint32_t *count, *seg_start, *chunk_pre;
    bucket_sort_tables(w.sort_ws, N, M, &count, &seg_start, &chunk_pre);

    const size_t xe = dtype_size(x_dtype);
    const bool al16 = is_aligned(X, 16) && ((ldx * xe) % 16 == 0);   // (whole 16-byte pieces stay inside their row)
    const dim3 grid((unsigned)w.maxchunks), block(FT);
#define DBGSOM_SEGSUM_MASKED(XT, V)                                                                               \
    hipLaunchKernelGGL((segsum_masked_kernel<XT, V>), grid, block, 0, s, (const XT *)X, di, ldx, w.order, kw, dist, \
                       seg_start, count, chunk_pre, Mi, w.slab)
    if (x_dtype == DBGSOM_F32) { if (al16) DBGSOM_SEGSUM_MASKED(float, 4); else DBGSOM_SEGSUM_MASKED(float, 1); }
    else { if (al16) DBGSOM_SEGSUM_MASKED(double, 2); else DBGSOM_SEGSUM_MASKED(double, 1); }
#undef DBGSOM_SEGSUM_MASKED
    const int NG = masked_groups(M);
    const int64_t W3 = 3 * d + 2;
    const unsigned col_blocks = (unsigned)((W3 + FT - 1) / FT < 8 ? (W3 + FT - 1) / FT : 8);
    hipLaunchKernelGGL(finalize_masked_kernel, dim3((unsigned)M, (unsigned)NG, col_blocks), dim3(FT), 0, s, w.slab, di, Mi,
                       chunk_pre, NG, w.gslab, sums);
    if (NG > 1)
        hipLaunchKernelGGL(finalize_masked_groups_kernel, dim3((unsigned)M, col_blocks), dim3(FT), 0, s, w.gslab, di, Mi, NG,
                           sums);
    return launch_status("masked accumulate kernels");
}

}  // namespace dbgsom

using namespace dbgsom;

extern "C" {

size_t dbgsom_accumulate_masked_workspace_bytes(int64_t N, int64_t d, int64_t M) {
    return accumulate_masked_workspace_bytes(N, d, M);
}

int dbgsom_accumulate_masked(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx, const int64_t *idx_dev,
                             const double *kw_dev, const double *dist_dev, int64_t M, double *sums_dev,
                             int32_t *status_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    return launch_accumulate_masked(X_dev, x_dtype, N, d, ldx, idx_dev, kw_dev, dist_dev, M, sums_dev, status_dev,
                                    workspace_dev, workspace_bytes, (hipStream_t)stream);
}

size_t dbgsom_smooth_masked_workspace_bytes(int64_t M, int64_t d) { return smooth_masked_workspace_bytes(M, d); }

int dbgsom_smooth_masked(const double *sums_dev, int64_t M, int64_t d, const float *hop_dev, double sigma,
                         const double *W_old_dev, double *W_new_dev, double *change_total_dev, void *workspace_dev,
                         size_t workspace_bytes, void *stream) {
    return launch_smooth_masked(sums_dev, M, d, hop_dev, sigma, W_old_dev, W_new_dev, change_total_dev, workspace_dev,
                                workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
