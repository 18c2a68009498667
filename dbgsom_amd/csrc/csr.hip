// CSR samples on gfx950: row norms, best-matching-unit search, per-neuron partial sums and the
// expansion into padded dense rows.
//
// Canonical CSR on the device: indptr int64 (N + 1), indices int32 ascending within a row and without
// duplicates, data float32 or float64 (explicitly stored zeros allowed).  Every dot product of this
// library is the sequential chain acc = fma(x_k, w_k, acc), k ascending (oracle/bmu_chain.c), and every
// per-neuron sum is added in list order (accumulate.hip).  A term with x_k == 0 leaves such a chain
// exactly where it was, so a kernel that walks only the stored entries of a row, in ascending column
// order, produces the bits the dense kernels produce on the densified matrix:
//
//   * row norms: the chain of row_sqnorms_kernel over the stored entries;
//   * search: r_ij = (xx_i + (-2 acc_ij)) + ww_j with acc_ij the chain over the stored entries against
//     Wt[col][j], a transposed float64 copy of the prototypes (d x ldwt, ldwt = M rounded up to the
//     workgroup size, zeros behind column M): one stored entry reads a contiguous run of prototypes.
//     Lanes own prototypes and hold the accumulators in registers; a workgroup walks CR rows at a time
//     (CR independent chains in flight per lane) and the (column, value) pairs of a row are uniform
//     across the workgroup.  More than 256 prototypes go in blocks of 256, ascending, so that a lane
//     meets its candidates with ascending index and the strict '<' of Best<K> keeps the lowest one.
//     The epilogue is that of bmu_kernel: clamp at 0, NaN never wins, ties to the lowest j, sqrt, the
//     optional float32 rounding (DBGSOM_STORE_WINNERS with RootFinish, direct_rows.h);
//   * sums: the CSR sibling of segsum_kernel -- one workgroup per chunk of <= CH rows of one neuron,
//     rows in list order, each stored entry added to its column's partial with the fused multiply-add
//     that segsum_kernel's `acc += w * v` compiles to (v_fmac_f64).  A slab row is d float64 wide and
//     does not fit LDS for wide data: the partials live in the slab row itself, zeroed by its owner,
//     rows visited one after the other with a barrier between them, distinct columns within a row --
//     no atomics, no races.  The counting sort in front and the two finalize passes behind are the
//     dense pipeline's own (accumulate.hip).
#include <math.h>

#include "direct_rows.h"

namespace dbgsom {

constexpr int CR = 4;      // rows per workgroup of the search = independent chains per lane
constexpr int CT = 256;    // threads per workgroup (= prototypes per block of the search)
constexpr int CCH = 128;   // rows per chunk of the sums: accumulate.hip's CH
static_assert(CT == MT, "the winners' tail of direct_rows.h is that of a workgroup of MT lanes");

int64_t csr_wt_ld(int64_t M) { return (M + CT - 1) / CT * CT; }

// ---- row norms ----------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(CT) void csr_row_sqnorms_kernel(const int64_t *__restrict__ indptr,
                                                             const T *__restrict__ data, int64_t N,
                                                             double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * CT + threadIdx.x;
    if (i >= N) return;
    double acc = 0.0;
    for (int64_t p = indptr[i], e = indptr[i + 1]; p < e; ++p) {
        const double v = widen(data[p]);
        acc = fma(v, v, acc);
    }
    out[i] = acc;
}

// ---- Wt[c][j] = W[j][c] (zeros for j >= M) --------------------------------------------------------
__global__ __launch_bounds__(256) void transpose_weights_kernel(const double *__restrict__ W, int M, int d,
                                                                int64_t ldw, double *__restrict__ Wt,
                                                                int64_t ldwt) {
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    const int j0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int j = j0 + ty + 8 * u, c = c0 + tx;
        tile[ty + 8 * u][tx] = (j < M && c < d) ? W[(int64_t)j * ldw + c] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int c = c0 + ty + 8 * u, j = j0 + tx;
        if (c < d && j < ldwt) Wt[(int64_t)c * ldwt + j] = tile[tx][ty + 8 * u];
    }
}

// ---- search -------------------------------------------------------------------------------------
template <typename T, int K>
__global__ __launch_bounds__(CT) void bmu_csr_kernel(
    const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices, const T *__restrict__ data,
    int64_t N, const double *__restrict__ xx, const double *__restrict__ Wt, int64_t ldwt, int M,
    const double *__restrict__ ww, int round_f32, int64_t *__restrict__ idx_out, double *__restrict__ dist_out) {
    const int tid = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * CR;
    int64_t p0[CR];
    int len[CR];
    double xi[CR];
    int maxlen = 0;
#pragma unroll
    for (int r = 0; r < CR; ++r) {
        const int64_t i = i0 + r;
        p0[r] = 0; len[r] = 0; xi[r] = 0.0;
        if (i < N) {
            p0[r] = indptr[i];
            len[r] = (int)(indptr[i + 1] - p0[r]);
            xi[r] = xx[i];
        }
        maxlen = max(maxlen, len[r]);
    }
    Best<K> best[CR];
#pragma unroll
    for (int r = 0; r < CR; ++r) best[r].init();

    for (int jb = 0; jb < M; jb += CT) {
        const int j = jb + tid;            // (j < ldwt: the columns behind M hold zeros)
        const double *__restrict__ wcol = Wt + j;
        double acc[CR];
#pragma unroll
        for (int r = 0; r < CR; ++r) acc[r] = 0.0;
        for (int e = 0; e < maxlen; ++e) {
#pragma unroll
            for (int r = 0; r < CR; ++r) {
                if (e < len[r]) {          // (uniform: the pair is the same for every lane)
                    const int c = indices[p0[r] + e];
                    const double v = widen(data[p0[r] + e]);
                    acc[r] = fma(v, wcol[(int64_t)c * ldwt], acc[r]);
                }
            }
        }
        if (j < M) {
            const double y = ww[j];
#pragma unroll
            for (int r = 0; r < CR; ++r) {
                double rv = (xi[r] + (-2.0 * acc[r])) + y;
                if (!(rv > 0.0)) rv = (rv != rv) ? rv : 0.0;  // max(r, 0), NaN kept
                best[r].push(rv, j);
            }
        }
    }
    const int nrows = (int)min((int64_t)CR, N - i0);
    const RootFinish fin{round_f32};
    DBGSOM_STORE_WINNERS(K, CR, best, i0, nrows, 0, fin, idx_out, dist_out);
}

// ---- sums: one workgroup sums one chunk (<= CCH rows of one neuron) in list order -------------------
// (the preamble, the scalar partials and the weighted form are segsum_kernel's, statement for statement)
template <typename T, bool WGT>
__global__ __launch_bounds__(CT) void segsum_csr_kernel(
    const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices, const T *__restrict__ data, int d,
    const int32_t *__restrict__ order, const double *__restrict__ kw, double gamma,
    const double *__restrict__ dist, const uint32_t *__restrict__ seg_start, const uint32_t *__restrict__ count,
    const uint32_t *__restrict__ chunk_pre, int M, double *slab, const double *__restrict__ sw) {
    constexpr int NS = WGT ? 3 : 2;   // scalar partials behind the d columns of a slab row
    __shared__ int32_t rows_s[CCH];
    __shared__ double kw_s[CCH];
    __shared__ double dist_s[CCH];
    __shared__ double sw_s[WGT ? CCH : 1];
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
        const uint32_t begin = seg_start[lo] + (c - chunk_pre[lo]) * CCH;
        const uint32_t end = min(begin + (uint32_t)CCH, seg_start[lo] + count[lo]);
        info[0] = begin; info[1] = end - begin;
    }
    double *out = slab + (size_t)c * (d + NS);
    for (int col = tid; col < d; col += CT) out[col] = 0.0;   // the owner zeroes its slab row
    __syncthreads();
    const uint32_t begin = info[0];
    const int n = (int)info[1];
    if (tid < n) {
        const int32_t r = order[begin + tid];
        rows_s[tid] = r;
        const double dd = dist[r];
        const double h = kw ? kw[r] : 1.0 - sqrt(1.0 - exp(-gamma * (dd * dd)));
        if constexpr (WGT) {
            const double w = sw[r];
            sw_s[tid] = w;
            kw_s[tid] = __dmul_rn(w, h);
            dist_s[tid] = __dmul_rn(w, dd);
        } else {
            kw_s[tid] = h;
            dist_s[tid] = dd;
        }
    }
    __syncthreads();
    if (tid == CT - 1) {  // the scalar partials, in list order
        double sk = 0.0, se = 0.0;
        for (int p = 0; p < n; ++p) { sk += kw_s[p]; se += dist_s[p]; }
        out[d] = sk;
        out[d + 1] = se;
        if constexpr (WGT) {
            double sa = 0.0;
            for (int p = 0; p < n; ++p) sa += sw_s[p];
            out[d + 2] = sa;
        }
    }
    for (int p = 0; p < n; ++p) {
        if constexpr (WGT) { if (sw_s[p] == 0.0) continue; }   // (weight 0: not streamed; uniform)
        const int64_t b = indptr[rows_s[p]], e = indptr[rows_s[p] + 1];
        const double w = kw_s[p];
        for (int64_t q = b + tid; q < e; q += CT) {
            const int col = indices[q];                     // distinct columns within a row
            out[col] = fma(w, widen(data[q]), out[col]);
        }
        __syncthreads();   // the next row may meet this row's columns in other lanes
    }
}

// ---- csr -> padded dense rows (the output is zero-filled by the caller) ------------------------------
template <typename T>
__global__ __launch_bounds__(64) void csr_densify_kernel(const int64_t *__restrict__ indptr,
                                                         const int32_t *__restrict__ indices,
                                                         const T *__restrict__ data, int64_t N, int64_t ld,
                                                         T *__restrict__ out) {
    for (int64_t i = blockIdx.x; i < N; i += gridDim.x)
        for (int64_t p = indptr[i] + threadIdx.x, e = indptr[i + 1]; p < e; p += 64)
            out[i * ld + indices[p]] = data[p];
}

// rows `ids` of the matrix as dense float64 rows of `cols` values
template <typename T>
__global__ __launch_bounds__(CT) void csr_rows_to_f64_kernel(const int64_t *__restrict__ indptr,
                                                             const int32_t *__restrict__ indices,
                                                             const T *__restrict__ data,
                                                             const int64_t *__restrict__ ids, int64_t n,
                                                             int64_t cols, double *dst) {
    const int64_t r = blockIdx.x;
    if (r >= n) return;
    double *o = dst + r * cols;
    for (int64_t c = threadIdx.x; c < cols; c += CT) o[c] = 0.0;
    __syncthreads();
    const int64_t i = ids[r];
    for (int64_t p = indptr[i] + threadIdx.x, e = indptr[i + 1]; p < e; p += CT) o[indices[p]] = widen(data[p]);
}

// -------------------------------------------------------------------------------------------------
static bool csr_dtype_ok(int dt) { return dt == DBGSOM_F32 || dt == DBGSOM_F64; }

int launch_csr_row_sqnorms(const CsrView &x, int dtype, int64_t N, double *out, hipStream_t s) {
    DBGSOM_REQUIRE(csr_dtype_ok(dtype), "CSR data must be DBGSOM_F32 or DBGSOM_F64");
    DBGSOM_REQUIRE(N >= 0 && N < 0x7fffffff, "bad shape");
    if (N == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(x.indptr && out, "null pointer");
    dim3 grid((unsigned)((N + CT - 1) / CT));
    if (dtype == DBGSOM_F32)
        hipLaunchKernelGGL(csr_row_sqnorms_kernel<float>, grid, dim3(CT), 0, s, x.indptr, (const float *)x.data, N, out);
    else
        hipLaunchKernelGGL(csr_row_sqnorms_kernel<double>, grid, dim3(CT), 0, s, x.indptr, (const double *)x.data, N, out);
    return launch_status("csr_row_sqnorms_kernel");
}

int launch_transpose_weights(const double *W, int64_t M, int64_t d, int64_t ldw, double *Wt, int64_t ldwt,
                             hipStream_t s) {
    DBGSOM_REQUIRE(M >= 1 && M <= 0x7fffff00 && d >= 1 && d <= 0x7fffffff && ldw >= d && ldwt >= M, "bad shape");
    DBGSOM_REQUIRE(ldwt == csr_wt_ld(M), "ldwt must be dbgsom_csr_wt_ld(M)");
    DBGSOM_REQUIRE(W && Wt, "null pointer");
    const int64_t gy = (d + 31) / 32;
    // (gridDim.y is limited to 65535: wide data goes in several launches of column ranges)
    for (int64_t y0 = 0; y0 < gy; y0 += 65535) {
        const int64_t ny = gy - y0 < 65535 ? gy - y0 : 65535;
        const int64_t c0 = y0 * 32;
        const int64_t dc = d - c0 < ny * 32 ? d - c0 : ny * 32;
        hipLaunchKernelGGL(transpose_weights_kernel, dim3((unsigned)(ldwt / 32), (unsigned)ny), dim3(256), 0, s,
                           W + c0, (int)M, (int)dc, ldw, Wt + c0 * ldwt, ldwt);
    }
    return launch_status("transpose_weights_kernel");
}

int launch_bmu_csr(const CsrView &x, int dtype, int64_t N, const double *xx, const double *Wt, int64_t ldwt,
                   int64_t M, const double *ww, int k, int round_f32, int64_t *idx, double *dist, hipStream_t s) {
    DBGSOM_REQUIRE(csr_dtype_ok(dtype), "CSR data must be DBGSOM_F32 or DBGSOM_F64");
    DBGSOM_REQUIRE(k == 1 || k == 2, "k must be 1 or 2");
    DBGSOM_REQUIRE(N >= 0 && N < 0x7fffffff, "bad sample shape");
    DBGSOM_REQUIRE(M >= k && M <= 0x7fffff00, "need k <= M < 2^31");
    DBGSOM_REQUIRE(ldwt == csr_wt_ld(M), "ldwt must be dbgsom_csr_wt_ld(M)");
    if (N == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(x.indptr && xx && Wt && ww && idx && dist, "null pointer");
    dim3 grid((unsigned)((N + CR - 1) / CR)), block(CT);
#define DBGSOM_BMU_CSR(T, KK)                                                                              \
    hipLaunchKernelGGL((bmu_csr_kernel<T, KK>), grid, block, 0, s, x.indptr, x.indices, (const T *)x.data, N, \
                       xx, Wt, ldwt, (int)M, ww, round_f32, idx, dist)
    if (dtype == DBGSOM_F32) { if (k == 1) DBGSOM_BMU_CSR(float, 1); else DBGSOM_BMU_CSR(float, 2); }
    else { if (k == 1) DBGSOM_BMU_CSR(double, 1); else DBGSOM_BMU_CSR(double, 2); }
#undef DBGSOM_BMU_CSR
    return launch_status("bmu_csr_kernel");
}

int launch_segsum_csr(const CsrView &x, int dtype, int64_t d, const int32_t *order, const double *kw, double gamma,
                      const double *dist, const uint32_t *seg_start, const uint32_t *count,
                      const uint32_t *chunk_pre, int64_t M, double *slab, const double *sw, int64_t maxchunks,
                      hipStream_t s) {
    DBGSOM_REQUIRE(csr_dtype_ok(dtype), "CSR data must be DBGSOM_F32 or DBGSOM_F64");
    DBGSOM_REQUIRE(x.indptr, "null CSR arrays");
    dim3 grid((unsigned)maxchunks), block(CT);
#define DBGSOM_SEGSUM_CSR(T, WG)                                                                            \
    hipLaunchKernelGGL((segsum_csr_kernel<T, WG>), grid, block, 0, s, x.indptr, x.indices, (const T *)x.data, \
                       (int)d, order, kw, gamma, dist, seg_start, count, chunk_pre, (int)M, slab, sw)
    if (dtype == DBGSOM_F32) { if (sw) DBGSOM_SEGSUM_CSR(float, true); else DBGSOM_SEGSUM_CSR(float, false); }
    else { if (sw) DBGSOM_SEGSUM_CSR(double, true); else DBGSOM_SEGSUM_CSR(double, false); }
#undef DBGSOM_SEGSUM_CSR
    return DBGSOM_OK;
}

int launch_csr_densify(const CsrView &x, int dtype, int64_t N, int64_t d, int64_t ld, void *out, hipStream_t s) {
    DBGSOM_REQUIRE(csr_dtype_ok(dtype), "CSR data must be DBGSOM_F32 or DBGSOM_F64");
    DBGSOM_REQUIRE(N >= 0 && d >= 1 && ld >= d, "bad shape");
    if (N == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(x.indptr && out, "null pointer");
    DBGSOM_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)N * ld * dtype_size(dtype), s));
    dim3 grid((unsigned)(N < 65536 ? N : 65536));
    if (dtype == DBGSOM_F32)
        hipLaunchKernelGGL(csr_densify_kernel<float>, grid, dim3(64), 0, s, x.indptr, x.indices, (const float *)x.data, N, ld, (float *)out);
    else
        hipLaunchKernelGGL(csr_densify_kernel<double>, grid, dim3(64), 0, s, x.indptr, x.indices, (const double *)x.data, N, ld, (double *)out);
    return launch_status("csr_densify_kernel");
}

int launch_csr_rows_to_f64(const CsrView &x, int dtype, const int64_t *ids, int64_t n, int64_t cols, double *dst,
                           hipStream_t s) {
    DBGSOM_REQUIRE(csr_dtype_ok(dtype), "CSR data must be DBGSOM_F32 or DBGSOM_F64");
    if (n == 0) return DBGSOM_OK;
    if (dtype == DBGSOM_F32)
        hipLaunchKernelGGL(csr_rows_to_f64_kernel<float>, dim3((unsigned)n), dim3(CT), 0, s, x.indptr, x.indices, (const float *)x.data, ids, n, cols, dst);
    else
        hipLaunchKernelGGL(csr_rows_to_f64_kernel<double>, dim3((unsigned)n), dim3(CT), 0, s, x.indptr, x.indices, (const double *)x.data, ids, n, cols, dst);
    return launch_status("csr_rows_to_f64_kernel");
}

}  // namespace dbgsom

using namespace dbgsom;

extern "C" {

// host only: needs no GPU
int dbgsom_csr_check(const int64_t *indptr_host, const int32_t *indices_host, int64_t N, int64_t d, int64_t nnz) {
    DBGSOM_REQUIRE(N >= 0 && d >= 1 && nnz >= 0, "bad shape");
    DBGSOM_REQUIRE(indptr_host && (indices_host || nnz == 0), "null pointer");
    if (indptr_host[0] != 0) { set_error("dbgsom_csr_check: indptr[0] is %lld, not 0", (long long)indptr_host[0]); return DBGSOM_EINVAL; }
    for (int64_t i = 0; i < N; ++i)
        if (indptr_host[i + 1] < indptr_host[i]) {
            set_error("dbgsom_csr_check: indptr is not monotone at row %lld (%lld after %lld)", (long long)i,
                      (long long)indptr_host[i + 1], (long long)indptr_host[i]);
            return DBGSOM_EINVAL;
        }
    if (indptr_host[N] != nnz) {
        set_error("dbgsom_csr_check: indptr[N] is %lld, not nnz = %lld", (long long)indptr_host[N], (long long)nnz);
        return DBGSOM_EINVAL;
    }
    for (int64_t i = 0; i < N; ++i)
        for (int64_t p = indptr_host[i]; p < indptr_host[i + 1]; ++p) {
            const int64_t c = indices_host[p];
            if (c < 0 || c >= d) {
                set_error("dbgsom_csr_check: column index %lld of row %lld is out of range [0, %lld)", (long long)c,
                          (long long)i, (long long)d);
                return DBGSOM_EINVAL;
            }
            if (p > indptr_host[i] && indices_host[p - 1] >= indices_host[p]) {
                set_error("dbgsom_csr_check: column indices of row %lld are not strictly ascending (%lld then %lld)",
                          (long long)i, (long long)indices_host[p - 1], (long long)c);
                return DBGSOM_EINVAL;
            }
        }
    return DBGSOM_OK;
}

int64_t dbgsom_csr_wt_ld(int64_t M) { return M < 1 ? 0 : csr_wt_ld(M); }

int dbgsom_csr_row_sqnorms(const int64_t *indptr, const void *data, int x_dtype, int64_t N, double *out, void *stream) {
    return launch_csr_row_sqnorms(CsrView{indptr, nullptr, data}, x_dtype, N, out, (hipStream_t)stream);
}

int dbgsom_csr_transpose_weights(const double *W, int64_t M, int64_t d, int64_t ldw, double *Wt, int64_t ldwt,
                                 void *stream) {
    return launch_transpose_weights(W, M, d, ldw, Wt, ldwt, (hipStream_t)stream);
}

int dbgsom_bmu_csr(const int64_t *indptr, const int32_t *indices, const void *data, int x_dtype, int64_t N,
                   const double *xx, const double *Wt, int64_t ldwt, int64_t M, const double *ww, int k, int round_f32,
                   int64_t *idx, double *dist, void *stream) {
    return launch_bmu_csr(CsrView{indptr, indices, data}, x_dtype, N, xx, Wt, ldwt, M, ww, k, round_f32, idx, dist,
                          (hipStream_t)stream);
}

int dbgsom_csr_densify(const int64_t *indptr, const int32_t *indices, const void *data, int x_dtype, int64_t N,
                       int64_t d, int64_t ld, void *out, void *stream) {
    return launch_csr_densify(CsrView{indptr, indices, data}, x_dtype, N, d, ld, out, (hipStream_t)stream);
}

size_t dbgsom_accumulate_csr_workspace_bytes(int64_t N, int64_t d, int64_t M) {
    return accumulate_weighted_workspace_bytes(N, d, M);   // (covers the unweighted form: its slab rows are one scalar narrower)
}

int dbgsom_accumulate_csr(const int64_t *indptr, const int32_t *indices, const void *data, int x_dtype, int64_t N,
                          int64_t d, const int64_t *idx, const double *kw, const double *sw, const double *dist,
                          int64_t M, double *sums, int32_t *status, void *ws, size_t ws_bytes, void *stream) {
    DBGSOM_REQUIRE(N == 0 || kw, "null sample weights");
    return launch_accumulate_csr(CsrView{indptr, indices, data}, x_dtype, N, d, idx, kw, 0.0, sw, dist, M, sums, status,
                                 false, ws, ws_bytes, (hipStream_t)stream);
}

}  // extern "C"
