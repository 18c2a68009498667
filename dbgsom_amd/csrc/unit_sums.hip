// Per-unit sums of a per-row quantity on gfx950 (MI355X): sums[j, v] = sum over the rows i of unit j of z_iv (or
// w_i z_iv), mass[j] = their number (or summed weight), in an order NumPy restates bit for bit; and the deviations of
// rows from their unit's centre.  What carries a target, an external variable or a measurement onto the map.
//
// The order.  The list L_j of unit j holds the rows i with unit[i] == j, ascending in i, without the rows of weight 0
// (scikit-learn's meaning of weight 0: a NaN stored under it is never read).  A row's term is z_iv, or the rounded
// product w_i * z_iv (never fused into the add); its mass term 1.0 or w_i.  L_j is cut into blocks of UNIT_CH = 128
// consecutive list positions -- the chunk length of accumulate.hip, so launch_bucket_sort's chunk_pre table is the
// table of blocks -- and
//   P[b][v]    = (((+0.0 + t_0) + t_1) + ...)          the terms of block b in list order, every add rounded
//   sums[j][v] = (((+0.0 + P[0][v]) + P[1][v]) + ...)  the blocks of unit j ascending; mass[j] likewise
// An empty list gives +0.0.  A row whose unit lies outside [0, M) is in no list.  NaN and infinities are plain IEEE.
//
// Kernels, on one stream:
//   0. unit_keys_kernel (weights only): key_i = unit_i, or -1 under weight 0 -- the sort then files the row nowhere;
//   1. launch_bucket_sort (accumulate.hip): the stable order by key, segment starts, chunk_pre;
//   2. unit_block_kernel: one wavefront per block, UNIT_WPB blocks per workgroup.  The block's terms are gathered
//      through `order` into LDS by all 64 lanes, 64 list rows at a time (64 x (V + 1) doubles per wavefront: 8.5 KiB
//      at V = 16, 34 KiB per workgroup, four workgroups per CU), element e = lane + 64 k of the row-major tile per
//      lane: consecutive lanes read consecutive doubles of a row of Z and write consecutive LDS words.  Lanes 0 .. V
//      (V values and the mass) then run their chain down the tile: lane v reads word r (V + 1) + v, a stride of one
//      double between lanes, no bank conflict;
//   3. unit_fold_kernel: one lane per (unit, column) adds that unit's partials, blocks ascending -- at M = 4 and
//      N = 1e6 that is 1954 dependent adds per lane where a flat chain would be 250 000.
// unit_deviations_kernel is elementwise: (y_iv - C_jv)^2 per entry, or the root of their sum over v ascending.
#include <math.h>

#include <algorithm>

#include "common.h"

namespace dbgsom {

constexpr int UNIT_CH = 128;    // list positions per block: CH of accumulate.hip (checked in launch_unit_sums)
constexpr int UNIT_HALF = 64;   // list rows per LDS tile
constexpr int UNIT_WPB = 4;     // wavefronts = blocks per workgroup
constexpr int UNIT_MAXV = 16;   // DBGSOM_MAX_MIXTURE_VALUES

__global__ __launch_bounds__(256) void unit_keys_kernel(const int64_t *__restrict__ unit, const double *__restrict__ w,
                                                        int64_t N, int64_t *__restrict__ key) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < N) key[i] = (w[i] == 0.0) ? (int64_t)-1 : unit[i];
}

__global__ __launch_bounds__(UNIT_WPB * 64) void unit_block_kernel(
    const int32_t *__restrict__ order, const uint32_t *__restrict__ seg_start, const uint32_t *__restrict__ count,
    const uint32_t *__restrict__ chunk_pre, int M, const double *__restrict__ Z, int64_t ldz,
    const double *__restrict__ w, int V, double *__restrict__ P) {
#pragma clang fp contract(off)
    __shared__ double tile[UNIT_WPB][UNIT_HALF * (UNIT_MAXV + 1)];
    __shared__ int32_t rows[UNIT_WPB][UNIT_HALF];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int Vp = V + 1;
    const uint32_t c = blockIdx.x * UNIT_WPB + wv;
    const bool live = c < chunk_pre[M];   // (uniform per wavefront; every wavefront meets every barrier)
    uint32_t begin = 0;
    int n = 0;
    if (live) {
        int lo = 0, hi = M;  // last j with chunk_pre[j] <= c: the one unit with a block c
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (chunk_pre[mid] <= c) lo = mid; else hi = mid;
        }
        begin = seg_start[lo] + (c - chunk_pre[lo]) * UNIT_CH;
        n = (int)(min(begin + (uint32_t)UNIT_CH, seg_start[lo] + count[lo]) - begin);
    }
    double acc = 0.0;
    double *t = tile[wv];
#pragma unroll 1
    for (int h = 0; h < UNIT_CH / UNIT_HALF; ++h) {
        const int m = min(max(n - h * UNIT_HALF, 0), UNIT_HALF);   // list rows of this tile
        if (lane < m) rows[wv][lane] = order[begin + h * UNIT_HALF + lane];
        __syncthreads();
        for (int e = lane; e < m * Vp; e += 64) {
            const int r = e / Vp, v = e - r * Vp;
            const int64_t i = rows[wv][r];
            double x;
            if (v < V) {
                x = Z[i * ldz + v];
                if (w) x = w[i] * x;
            } else {
                x = w ? w[i] : 1.0;
            }
            t[e] = x;
        }
        __syncthreads();
        if (lane < Vp)
            for (int r = 0; r < m; ++r) acc = acc + t[r * Vp + lane];
        __syncthreads();   // (the tile is rewritten by the next round)
    }
    if (live && lane < Vp) P[(size_t)c * Vp + lane] = acc;
}

__global__ __launch_bounds__(256) void unit_fold_kernel(const double *__restrict__ P, const uint32_t *__restrict__ chunk_pre,
                                                        int M, int V, double *__restrict__ mass, double *__restrict__ sums,
                                                        int64_t lds) {
#pragma clang fp contract(off)
    const int Vp = V + 1;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)M * Vp) return;
    const int j = (int)(e / Vp), v = (int)(e - (int64_t)j * Vp);
    const uint32_t b0 = chunk_pre[j], b1 = chunk_pre[j + 1];
    double acc = 0.0;
    uint32_t b = b0;
    for (; b + 8 <= b1; b += 8) {   // eight independent loads in flight, the adds in order
        double x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = P[(size_t)(b + u) * Vp + v];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = acc + x[u];
    }
    for (; b < b1; ++b) acc = acc + P[(size_t)b * Vp + v];
    if (v < V) sums[(int64_t)j * lds + v] = acc;
    else mass[j] = acc;
}

__global__ __launch_bounds__(256) void unit_zero_kernel(int64_t M, int V, double *__restrict__ mass, double *__restrict__ sums,
                                                        int64_t lds) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= M * (V + 1)) return;
    const int64_t j = e / (V + 1);
    const int v = (int)(e - j * (V + 1));
    if (v < V) sums[j * lds + v] = 0.0;
    else mass[j] = 0.0;
}

template <int MODE>
__global__ __launch_bounds__(256) void unit_deviations_kernel(const int64_t *__restrict__ unit, const double *__restrict__ Y,
                                                              int64_t ldy, int64_t N, const double *__restrict__ C,
                                                              int64_t ldc, int64_t M, int V, double *__restrict__ out,
                                                              int64_t ldo) {
#pragma clang fp contract(off)
    if constexpr (MODE == DBGSOM_DEVIATIONS_SQUARES) {
        const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
        if (e >= N * V) return;
        const int64_t i = e / V;
        const int v = (int)(e - i * V);
        const int64_t j = unit[i];
        double r = 0.0;
        if (j >= 0 && j < M) {
            const double df = Y[i * ldy + v] - C[j * ldc + v];
            r = df * df;
        }
        out[i * ldo + v] = r;
    } else {
        const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
        if (i >= N) return;
        const int64_t j = unit[i];
        double r = 0.0;
        if (j >= 0 && j < M) {
            double s = 0.0;
            for (int v = 0; v < V; ++v) {
                const double df = Y[i * ldy + v] - C[j * ldc + v];
                const double q = df * df;
                s = s + q;
            }
            r = __dsqrt_rn(s);
        }
        out[i] = r;
    }
}

static inline unsigned unit_grid(int64_t n) { return (unsigned)((n + 255) / 256); }

// blocks a call can have: every unit ends at most one block that is not full
static inline int64_t unit_max_blocks(int64_t N, int64_t M) { return N / UNIT_CH + std::min(N, M); }

// [keys: N int64 (weights only) | order: N int32 | the sort's workspace | P: blocks x (V + 1) float64]
size_t unit_sums_workspace_bytes(int64_t N, int64_t M, int V, bool weighted) {
    return (weighted ? align_up((size_t)N * 8) : 0) + align_up((size_t)N * 4) + align_up(bucket_sort_workspace_bytes(N, M)) +
           align_up((size_t)unit_max_blocks(N, M) * (V + 1) * 8);
}

int launch_unit_sums(const int64_t *unit, const double *Z, int64_t ldz, const double *w, int64_t N, int64_t M, int V,
                     double *mass, double *sums, int64_t lds, void *ws, size_t ws_bytes, hipStream_t s) {
    if (accumulate_chunk_rows() != UNIT_CH) { set_error("unit sums: the sort cuts blocks of another length"); return DBGSOM_EINVAL; }
    if (N == 0) {
        hipLaunchKernelGGL(unit_zero_kernel, dim3(unit_grid(M * (V + 1))), dim3(256), 0, s, M, V, mass, sums, lds);
        return launch_status("unit_zero_kernel");
    }
    const int rc = workspace_check("unit sums", ws_bytes, unit_sums_workspace_bytes(N, M, V, w != nullptr));
    if (rc != DBGSOM_OK) return rc;
    char *base = (char *)ws;
    const int64_t *keys = unit;
    if (w) {
        int64_t *k = (int64_t *)base;
        base += align_up((size_t)N * 8);
        hipLaunchKernelGGL(unit_keys_kernel, dim3(unit_grid(N)), dim3(256), 0, s, unit, w, N, k);
        keys = k;
    }
    int32_t *order = (int32_t *)base;
    base += align_up((size_t)N * 4);
    void *sort_ws = base;
    base += align_up(bucket_sort_workspace_bytes(N, M));
    double *P = (double *)base;
    const int rs = launch_bucket_sort(keys, N, M, order, sort_ws, s);
    if (rs != DBGSOM_OK) return rs;
    const uint32_t *count, *seg_start, *chunk_pre;
    bucket_sort_tables(sort_ws, N, M, &count, &seg_start, &chunk_pre);
    const int64_t blocks = unit_max_blocks(N, M);
    hipLaunchKernelGGL(unit_block_kernel, dim3((unsigned)((blocks + UNIT_WPB - 1) / UNIT_WPB)), dim3(UNIT_WPB * 64), 0, s,
                       (const int32_t *)order, seg_start, count, chunk_pre, (int)M, Z, ldz, w, V, P);
    hipLaunchKernelGGL(unit_fold_kernel, dim3(unit_grid(M * (V + 1))), dim3(256), 0, s, (const double *)P, chunk_pre, (int)M, V,
                       mass, sums, lds);
    return launch_status("unit sums kernels");
}

int launch_unit_deviations(const int64_t *unit, const double *Y, int64_t ldy, int64_t N, const double *C, int64_t ldc,
                           int64_t M, int V, int mode, double *out, int64_t ldo, hipStream_t s) {
    if (N == 0) return DBGSOM_OK;
    if (mode == DBGSOM_DEVIATIONS_SQUARES)
        hipLaunchKernelGGL(unit_deviations_kernel<DBGSOM_DEVIATIONS_SQUARES>, dim3(unit_grid(N * V)), dim3(256), 0, s, unit, Y,
                           ldy, N, C, ldc, M, V, out, ldo);
    else
        hipLaunchKernelGGL(unit_deviations_kernel<DBGSOM_DEVIATIONS_NORM>, dim3(unit_grid(N)), dim3(256), 0, s, unit, Y, ldy, N,
                           C, ldc, M, V, out, ldo);
    return launch_status("unit_deviations_kernel");
}

}  // namespace dbgsom
