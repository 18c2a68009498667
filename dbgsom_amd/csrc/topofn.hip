// The topographic function of a fitted map on gfx950 (MI355X): the graph stage of
// BaseSom.topographic_function / BaseSom.phi (reference dbgsom/BaseSom.py:955-998).
//
// The reference builds the "induced Delaunay" graph of the map (an edge {a, b} for every sample whose
// first and second BMU are a and b), runs Floyd-Warshall on it (O(M^3)) and counts pairs of neurons in
// dense M x M matrices.  What phi(k) needs is two integer histograms:
//   hist_pos[c]  ordered Delaunay edges (i, j) by the Chebyshev distance c of their lattice positions
//   hist_neg[t]  ordered lattice 4-neighbour pairs (i, j) by their hop distance t in the graph
//                (1 .. M - 1); hist_neg[M]: the pairs with no path between them
// so phi(k > 0) and phi(k < 0) are suffix sums of them.  Stages (DESIGN.md "Topographic function"):
//   1. edge set: a symmetric M x ceil(M/32) bitmap from the (n, 2) winner pairs; every word is read
//      before its atomicOr, so the hot edges (most samples fall on a few hundred pairs) do not
//      serialise on atomics.  Indices outside [0, M) set a status bit (DBGSOM_ERANGE).
//   2. CSR: one wave per row counts the row's bits, a one-workgroup scan gives the offsets, one wave per
//      row writes the neighbours in ascending order (deterministic).  The lattice 4-neighbour table
//      (M x 4, by coordinates over all pairs, as the reference's euclidean_distances == 1) is built here.
//   3. distances: a breadth-first search from every source, one source per workgroup, the visited set
//      and the queue in LDS; no communication between workgroups, every loop bounded by M levels.
//      Histogram mode stops a source once its lattice neighbours have distances (or its component is
//      exhausted); full mode writes the source's row of D (int32, -1 = unreachable).
//   4. histograms: integer counters (LDS bins, then global adds), so the result has no ordering question.
#include <algorithm>

#include "common.h"

namespace dbgsom {

namespace {

constexpr int TF_BLOCK = 256;
constexpr int TF_HB = 1024;           // LDS bins per histogram in the histogram kernel (the rest: global adds)
constexpr uint32_t TF_ST_RANGE = 1u;  // status bits: a winner index outside [0, M)
constexpr uint32_t TF_ST_NPOS = 2u;   //              a Chebyshev distance >= n_pos
constexpr uint32_t TF_ST_DUP = 4u;    //              two neurons with the same lattice coordinates

// 1. edge set ---------------------------------------------------------------------------------------
__device__ __forceinline__ void tf_set_bit(uint32_t *bm, int64_t W32, int64_t a, int64_t b) {
    uint32_t *w = bm + a * W32 + (b >> 5);
    const uint32_t bit = 1u << (b & 31);
    if (!(*w & bit)) atomicOr(w, bit);  // (a stale read only costs one atomic more)
}

__global__ __launch_bounds__(TF_BLOCK) void tf_edges_kernel(const int64_t *__restrict__ idx2, int64_t n, int64_t M,
                                                            int64_t W32, uint32_t *bm, uint32_t *status) {
    for (int64_t i = (int64_t)blockIdx.x * TF_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * TF_BLOCK) {
        const int64_t a = idx2[2 * i], b = idx2[2 * i + 1];
        if (a < 0 || a >= M || b < 0 || b >= M) {
            atomicOr(status, TF_ST_RANGE);
            continue;
        }
        if (a == b) continue;  // (no self-loops: D's diagonal is 0 either way)
        tf_set_bit(bm, W32, a, b);
        tf_set_bit(bm, W32, b, a);
    }
}

// 2. CSR --------------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_sum(int v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// degree of every row: rowptr[u + 1] (one wave per row)
__global__ __launch_bounds__(TF_BLOCK) void tf_row_count_kernel(const uint32_t *__restrict__ bm, int M, int W32,
                                                                int32_t *rowptr) {
    const int row = blockIdx.x * (TF_BLOCK / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;  // (whole waves)
    int c = 0;
    for (int w = lane; w < W32; w += 64) c += __popc(bm[(int64_t)row * W32 + w]);
    c = wave_sum(c);
    if (lane == 0) rowptr[row + 1] = c;
}

// rowptr[1..M] := inclusive prefix sums of the degrees, rowptr[0] := 0 (one workgroup of 1024)
__global__ __launch_bounds__(1024) void tf_scan_kernel(int32_t *rowptr, int M) {
    __shared__ int32_t part[1024];
    const int t = threadIdx.x;
    const int per = (M + 1023) / 1024;
    const int lo = std::min(M, t * per), hi = std::min(M, lo + per);
    int s = 0;
    for (int k = lo; k < hi; ++k) s += rowptr[k + 1];
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {  // Hillis-Steele inclusive scan of the chunk sums
        const int v = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - s;
    for (int k = lo; k < hi; ++k) {
        run += rowptr[k + 1];
        rowptr[k + 1] = run;
    }
    if (t == 0) rowptr[0] = 0;
}

// neighbour lists in ascending order (one wave per row; a wave-wide exclusive scan of the words' popcounts)
__global__ __launch_bounds__(TF_BLOCK) void tf_fill_kernel(const uint32_t *__restrict__ bm, int M, int W32,
                                                           const int32_t *__restrict__ rowptr, uint16_t *cols) {
    const int row = blockIdx.x * (TF_BLOCK / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    int base = rowptr[row];
    for (int w0 = 0; w0 < W32; w0 += 64) {
        const int w = w0 + lane;
        uint32_t word = w < W32 ? bm[(int64_t)row * W32 + w] : 0u;
        const int c = __popc(word);
        int incl = c;
        for (int off = 1; off < 64; off <<= 1) {
            const int v = __shfl_up(incl, off, 64);
            if (lane >= off) incl += v;
        }
        int pos = base + incl - c;
        while (word) {
            const int b = __ffs(word) - 1;
            cols[pos++] = (uint16_t)(w * 32 + b);
            word &= word - 1u;
        }
        base += __shfl(incl, 63, 64);
    }
}

// lattice 4-neighbours by coordinates over all pairs (|dx| + |dy| == 1 <=> euclidean distance 1 for
// integers); nb[4 i + s] = the neighbours in ascending index order, -1 behind them
__global__ __launch_bounds__(TF_BLOCK) void tf_lattice_kernel(const int32_t *__restrict__ xy, int M, int32_t *nb,
                                                              uint32_t *status) {
    __shared__ int32_t tx[TF_BLOCK], ty[TF_BLOCK];
    const int i = blockIdx.x * TF_BLOCK + threadIdx.x;
    const int64_t xi = i < M ? xy[2 * i] : 0, yi = i < M ? xy[2 * i + 1] : 0;
    int cnt = 0, f0 = -1, f1 = -1, f2 = -1, f3 = -1;
    bool dup = false;
    for (int base = 0; base < M; base += TF_BLOCK) {
        const int j = base + threadIdx.x;
        __syncthreads();
        if (j < M) {
            tx[threadIdx.x] = xy[2 * j];
            ty[threadIdx.x] = xy[2 * j + 1];
        }
        __syncthreads();
        const int n = std::min(TF_BLOCK, M - base);
        if (i < M) {
            for (int k = 0; k < n; ++k) {
                const int64_t dx = (int64_t)tx[k] - xi, dy = (int64_t)ty[k] - yi;
                const int64_t l1 = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy);
                if (l1 == 1) {
                    const int jj = base + k;
                    f0 = cnt == 0 ? jj : f0;
                    f1 = cnt == 1 ? jj : f1;
                    f2 = cnt == 2 ? jj : f2;
                    f3 = cnt == 3 ? jj : f3;
                    ++cnt;
                } else if (l1 == 0 && base + k != i) {
                    dup = true;
                }
            }
        }
    }
    if (i < M) {
        nb[4 * i] = f0;
        nb[4 * i + 1] = f1;
        nb[4 * i + 2] = f2;
        nb[4 * i + 3] = f3;
        if (dup || cnt > 4) atomicOr(status, TF_ST_DUP);
    }
}

// 3. distances: one source per workgroup ------------------------------------------------------------
// LDS: visited bits (W32 words) | queue (M uint16: every neuron enters once, levels are contiguous
// segments) | FULL: dist (M uint16, 0xffff = not reached)
template <bool FULL>
__global__ __launch_bounds__(TF_BLOCK) void tf_bfs_kernel(const int32_t *__restrict__ rowptr,
                                                          const uint16_t *__restrict__ cols,
                                                          const int32_t *__restrict__ nb, int M, int W32,
                                                          int32_t *D, int32_t *nbd) {
    extern __shared__ uint32_t tf_lds[];
    uint32_t *vis = tf_lds;
    uint16_t *queue = reinterpret_cast<uint16_t *>(vis + W32);
    uint16_t *dist = queue + ((M + 1) & ~1);
    __shared__ int s_lo, s_hi, s_tail, s_found, s_stop;
    __shared__ int s_nbd[4];
    const int src = blockIdx.x, t = threadIdx.x;
    const int n0 = nb[4 * src], n1 = nb[4 * src + 1], n2 = nb[4 * src + 2], n3 = nb[4 * src + 3];
    const int n_nb = (n0 >= 0) + (n1 >= 0) + (n2 >= 0) + (n3 >= 0);
    for (int k = t; k < W32; k += TF_BLOCK) vis[k] = 0u;
    if (FULL)
        for (int k = t; k < M; k += TF_BLOCK) dist[k] = 0xffff;
    if (t < 4) s_nbd[t] = -1;
    __syncthreads();
    if (t == 0) {
        vis[src >> 5] |= 1u << (src & 31);
        queue[0] = (uint16_t)src;
        if (FULL) dist[src] = 0;
        s_lo = 0;
        s_hi = 1;
        s_tail = 1;
        s_found = 0;
        s_stop = n_nb == 0 && !FULL;
    }
    __syncthreads();
    // level L discovers the neurons at distance L; distances are < M
    for (int L = 1; L < M && !s_stop; ++L) {
        const int lo = s_lo, hi = s_hi;
        for (int q = lo + t; q < hi; q += TF_BLOCK) {
            const int u = queue[q];
            const int e1 = rowptr[u + 1];
            for (int e = rowptr[u]; e < e1; ++e) {
                const int v = cols[e];
                const uint32_t bit = 1u << (v & 31);
                if (vis[v >> 5] & bit) continue;
                if (atomicOr(&vis[v >> 5], bit) & bit) continue;  // another lane claimed it
                queue[atomicAdd(&s_tail, 1)] = (uint16_t)v;
                if (FULL) dist[v] = (uint16_t)L;
                const int j = v == n0 ? 0 : v == n1 ? 1 : v == n2 ? 2 : v == n3 ? 3 : -1;
                if (j >= 0) {
                    s_nbd[j] = L;
                    atomicAdd(&s_found, 1);
                }
            }
        }
        __syncthreads();
        if (t == 0) {  // (only thread 0 writes these, between the two barriers; everyone reads them after)
            s_lo = hi;
            s_hi = s_tail;
            s_stop = s_tail == hi || (!FULL && s_found == n_nb);
        }
        __syncthreads();
    }
    if (t < 4) nbd[4 * src + t] = s_nbd[t];
    if (FULL) {
        int32_t *row = D + (int64_t)src * M;
        for (int k = t; k < M; k += TF_BLOCK) {
            const int v = dist[k];
            row[k] = v == 0xffff ? -1 : v;
        }
    }
}

// 4. histograms -------------------------------------------------------------------------------------
__device__ __forceinline__ void tf_count(uint32_t *lds_bins, unsigned long long *glob, int64_t b) {
    if (b < TF_HB) atomicAdd(&lds_bins[b], 1u);
    else atomicAdd(&glob[b], 1ull);
}

__global__ __launch_bounds__(TF_BLOCK) void tf_hist_kernel(const int32_t *__restrict__ rowptr,
                                                           const uint16_t *__restrict__ cols,
                                                           const int32_t *__restrict__ xy,
                                                           const int32_t *__restrict__ nb,
                                                           const int32_t *__restrict__ nbd, int M, int64_t n_pos,
                                                           unsigned long long *hist_pos, unsigned long long *hist_neg,
                                                           uint32_t *status) {
    __shared__ uint32_t hp[TF_HB], hn[TF_HB];
    for (int k = threadIdx.x; k < TF_HB; k += TF_BLOCK) hp[k] = hn[k] = 0u;
    __syncthreads();
    for (int s = blockIdx.x * TF_BLOCK + threadIdx.x; s < M; s += gridDim.x * TF_BLOCK) {
        const int64_t xs = xy[2 * s], ys = xy[2 * s + 1];
        const int e1 = rowptr[s + 1];
        for (int e = rowptr[s]; e < e1; ++e) {
            const int v = cols[e];
            const int64_t dx = (int64_t)xy[2 * v] - xs, dy = (int64_t)xy[2 * v + 1] - ys;
            const int64_t c = std::max(dx < 0 ? -dx : dx, dy < 0 ? -dy : dy);
            if (c >= n_pos) {
                atomicOr(status, TF_ST_NPOS);
                continue;
            }
            tf_count(hp, hist_pos, c);
        }
        for (int k = 0; k < 4; ++k) {
            if (nb[4 * s + k] < 0) continue;
            const int d = nbd[4 * s + k];
            tf_count(hn, hist_neg, d >= 0 ? d : M);
        }
    }
    __syncthreads();
    const int64_t np = std::min<int64_t>(n_pos, TF_HB), nn = std::min<int64_t>((int64_t)M + 1, TF_HB);
    for (int k = threadIdx.x; k < np; k += TF_BLOCK)
        if (hp[k]) atomicAdd(&hist_pos[k], (unsigned long long)hp[k]);
    for (int k = threadIdx.x; k < nn; k += TF_BLOCK)
        if (hn[k]) atomicAdd(&hist_neg[k], (unsigned long long)hn[k]);
}

// ---------------------------------------------------------------------------------------------------
struct TfWs {
    uint32_t *status, *bm;
    int32_t *rowptr, *nb, *nbd;
    uint16_t *cols;
};

size_t carve_ws(TfWs *w, char *base, int64_t M) {
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = base ? base + off : nullptr; off += align_up(bytes); return p; };
    const int64_t W32 = (M + 31) / 32;
    w->status = reinterpret_cast<uint32_t *>(take(256));
    w->bm = reinterpret_cast<uint32_t *>(take((size_t)M * W32 * 4));
    w->rowptr = reinterpret_cast<int32_t *>(take((size_t)(M + 1) * 4));
    w->nb = reinterpret_cast<int32_t *>(take((size_t)M * 16));
    w->nbd = reinterpret_cast<int32_t *>(take((size_t)M * 16));
    // every ordered pair of distinct neurons may be an edge (uint16: M <= DBGSOM_MAX_PROTOTYPES)
    w->cols = reinterpret_cast<uint16_t *>(take((size_t)std::max<int64_t>(1, M * (M - 1)) * 2));
    return off;
}

struct TfTimer {
    bool enabled = false, created = false;
    hipEvent_t ev[4];
    double ms[4] = {0, 0, 0, 0};  // search, edges + CSR, distances, histograms
};
TfTimer g_tf_timer;

}  // namespace

bool topofn_timing_enabled() { return g_tf_timer.enabled; }
void topofn_add_search_ms(double ms) { g_tf_timer.ms[0] += ms; }

}  // namespace dbgsom

using namespace dbgsom;

extern "C" {

size_t dbgsom_topofn_workspace_bytes(int64_t M, int full) {
    (void)full;  // (full mode writes into the caller's D; the workspace is the same)
    if (M < 1 || M > DBGSOM_MAX_PROTOTYPES) return 0;
    TfWs w;
    return carve_ws(&w, nullptr, M);
}

int dbgsom_topofn(const int64_t *idx2, int64_t n, const int32_t *xy, int64_t M, int64_t n_pos, uint64_t *hist_pos,
                  uint64_t *hist_neg, int32_t *D, void *ws, size_t ws_bytes, void *stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    DBGSOM_REQUIRE(M >= 1 && M <= DBGSOM_MAX_PROTOTYPES, "M must be in [1, DBGSOM_MAX_PROTOTYPES]");
    DBGSOM_REQUIRE(n >= 0 && n_pos >= 1, "bad shape");
    DBGSOM_REQUIRE(xy && hist_pos && hist_neg && (n == 0 || idx2), "null pointer");
    DBGSOM_REQUIRE(ws, "null pointer");
    DBGSOM_REQUIRE(is_aligned(ws, 256), "workspace must be 256-byte aligned");
    if (ws_bytes < dbgsom_topofn_workspace_bytes(M, D != nullptr)) {
        set_error("dbgsom_topofn: workspace too small");
        return DBGSOM_ENOMEM;
    }
    const bool full = D != nullptr;
    TfWs w;
    carve_ws(&w, static_cast<char *>(ws), M);
    const int Mi = (int)M, W32 = (int)((M + 31) / 32);
    TfTimer &tm = g_tf_timer;
    if (tm.enabled && !tm.created) {
        for (auto &e : tm.ev) DBGSOM_HIP_CHECK(hipEventCreate(&e));
        tm.created = true;
    }
    const bool timed = tm.enabled;
    auto stamp = [&](int i) { return timed ? hipEventRecord(tm.ev[i], stream) : hipSuccess; };
    DBGSOM_HIP_CHECK(stamp(0));
    DBGSOM_HIP_CHECK(hipMemsetAsync(w.status, 0, 4, stream));
    DBGSOM_HIP_CHECK(hipMemsetAsync(w.bm, 0, (size_t)M * W32 * 4, stream));
    if (n > 0) {
        const unsigned g = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + TF_BLOCK - 1) / TF_BLOCK, 4096));
        hipLaunchKernelGGL(tf_edges_kernel, dim3(g), dim3(TF_BLOCK), 0, stream, idx2, n, M, (int64_t)W32, w.bm,
                           w.status);
        if (const int rc = launch_status("tf_edges_kernel")) return rc;
    }
    const unsigned g_rows = (unsigned)((M + TF_BLOCK / 64 - 1) / (TF_BLOCK / 64));
    hipLaunchKernelGGL(tf_row_count_kernel, dim3(g_rows), dim3(TF_BLOCK), 0, stream, w.bm, Mi, W32, w.rowptr);
    if (const int rc = launch_status("tf_row_count_kernel")) return rc;
    hipLaunchKernelGGL(tf_scan_kernel, dim3(1), dim3(1024), 0, stream, w.rowptr, Mi);
    if (const int rc = launch_status("tf_scan_kernel")) return rc;
    hipLaunchKernelGGL(tf_fill_kernel, dim3(g_rows), dim3(TF_BLOCK), 0, stream, w.bm, Mi, W32, w.rowptr, w.cols);
    if (const int rc = launch_status("tf_fill_kernel")) return rc;
    hipLaunchKernelGGL(tf_lattice_kernel, dim3((unsigned)((M + TF_BLOCK - 1) / TF_BLOCK)), dim3(TF_BLOCK), 0, stream,
                       xy, Mi, w.nb, w.status);
    if (const int rc = launch_status("tf_lattice_kernel")) return rc;
    DBGSOM_HIP_CHECK(stamp(1));
    const size_t lds = (size_t)W32 * 4 + (size_t)((M + 1) & ~1) * 2 + (full ? (size_t)M * 2 : 0);
    if (full) {
        DBGSOM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&tf_bfs_kernel<true>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(tf_bfs_kernel<true>, dim3((unsigned)M), dim3(TF_BLOCK), lds, stream, w.rowptr, w.cols, w.nb,
                           Mi, W32, D, w.nbd);
    } else {
        DBGSOM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&tf_bfs_kernel<false>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(tf_bfs_kernel<false>, dim3((unsigned)M), dim3(TF_BLOCK), lds, stream, w.rowptr, w.cols,
                           w.nb, Mi, W32, nullptr, w.nbd);
    }
    if (const int rc = launch_status("tf_bfs_kernel")) return rc;
    DBGSOM_HIP_CHECK(stamp(2));
    DBGSOM_HIP_CHECK(hipMemsetAsync(hist_pos, 0, (size_t)n_pos * 8, stream));
    DBGSOM_HIP_CHECK(hipMemsetAsync(hist_neg, 0, (size_t)(M + 1) * 8, stream));
    const unsigned g_h = (unsigned)std::min<int64_t>((M + TF_BLOCK - 1) / TF_BLOCK, 256);
    hipLaunchKernelGGL(tf_hist_kernel, dim3(g_h), dim3(TF_BLOCK), 0, stream, w.rowptr, w.cols, xy, w.nb, w.nbd, Mi,
                       n_pos, reinterpret_cast<unsigned long long *>(hist_pos),
                       reinterpret_cast<unsigned long long *>(hist_neg), w.status);
    if (const int rc = launch_status("tf_hist_kernel")) return rc;
    DBGSOM_HIP_CHECK(stamp(3));
    // (blocking: the status word decides the return code)
    uint32_t status = 0;
    DBGSOM_HIP_CHECK(hipMemcpyAsync(&status, w.status, 4, hipMemcpyDeviceToHost, stream));
    DBGSOM_HIP_CHECK(hipStreamSynchronize(stream));
    if (timed) {
        float ms = 0.0f;
        for (int i = 0; i < 3; ++i) {
            DBGSOM_HIP_CHECK(hipEventElapsedTime(&ms, tm.ev[i], tm.ev[i + 1]));
            tm.ms[i + 1] += ms;
        }
    }
    if (status & TF_ST_RANGE) {
        set_error("dbgsom_topofn: a winner index outside [0, %lld)", (long long)M);
        return DBGSOM_ERANGE;
    }
    if (status & TF_ST_NPOS) {
        set_error("dbgsom_topofn: a Delaunay edge spans a Chebyshev distance >= n_pos = %lld", (long long)n_pos);
        return DBGSOM_EINVAL;
    }
    if (status & TF_ST_DUP) {
        set_error("dbgsom_topofn: two neurons share lattice coordinates");
        return DBGSOM_EINVAL;
    }
    return DBGSOM_OK;
}

int dbgsom_topofn_timing(int enable) {
    g_tf_timer.enabled = enable != 0;
    for (double &m : g_tf_timer.ms) m = 0.0;
    return DBGSOM_OK;
}

int dbgsom_topofn_stage_ms(double *ms4) {
    DBGSOM_REQUIRE(ms4, "null pointer");
    for (int i = 0; i < 4; ++i) ms4[i] = g_tf_timer.ms[i];
    return DBGSOM_OK;
}

}  // extern "C"
