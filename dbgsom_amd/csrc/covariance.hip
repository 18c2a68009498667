// One pass over dense rows that multiplies a block of directions by the (unnormalised) covariance of the rows:
// with c_ik = widen(x_ik) - mean_k (rounded once, float64)
//     y_ij = sum_k c_ik V_kj        Z_lj = sum_i c_il y_ij        s_l = sum_i c_il
// V and Z are d x p row-major float64, 1 <= p <= DBGSOM_MAX_DIRECTIONS.  What the linear initialisation
// (dbgsom_amd/linear_init.py) iterates: Z = C^T (C V), and with mean = 0 the column sums for the mean.
//
// Layout.  A workgroup of 256 threads owns a contiguous share of the rows and walks it CV_R rows at a time; thread t
// owns the columns t, t + 256, ... of a chunk of CW = 256 CPT columns (CPT = 1, 2, 4 for d <= 256, 512, 1024).  A step
// loads its CV_R x CPT elements once (one dword / qword per lane, consecutive lanes on consecutive columns, no
// alignment asked of the base or of ldx; d <= 1024: one step ahead, in flight across the step's barriers) and keeps them
// in registers for both products:
//   1. partial y over the thread's columns (V transposed in LDS, 8 x CW doubles, zero beyond p and d),
//   2. the CV_R x 8 partials of a wave folded with a halving butterfly (32 exchanges instead of 192: the lanes' halves
//      trade half of their values at every level; the two widest levels are v_permlane32_swap / v_permlane16_swap, the
//      rest shuffles), the four waves joined through LDS in a fixed order,
//   3. Z_lj += c_il y_ij and s_l += c_il for the thread's columns, the accumulators in registers.
// Every workgroup stores its Z and s as one partial [9][d] in the workspace; a second kernel adds the partials of an
// entry in order.  No atomics; the order of every sum is a function of (N, d) alone.  Eight directions are always
// computed (V padded with zeros), so the order does not depend on p either.
// d > 1024: the columns are cut into chunks of 1024 over blockIdx.y.  A workgroup then forms y over all chunks (V from
// global memory) and Z for its own chunk: the first product is repeated per chunk, the price of keeping one pass
// structure for widths no map in the benchmarks has.
#include "common.h"

namespace dbgsom {

constexpr int CV_T = 256, CV_R = 4, CV_P = DBGSOM_MAX_DIRECTIONS, CV_NV = CV_R * CV_P;
constexpr int CV_MAX_PARTIALS = 512, CV_MIN_SHARE = 64, CV_MAX_CPT = 4;
static_assert(CV_NV == 32 && CV_T == 256, "the butterfly below folds 32 values over 64 lanes, four waves");

// rows per workgroup and number of workgroups (= partials): functions of N alone
inline int64_t cov_share(int64_t N) {
    const int64_t even = ((N + CV_MAX_PARTIALS - 1) / CV_MAX_PARTIALS + CV_R - 1) / CV_R * CV_R;
    return even < CV_MIN_SHARE ? CV_MIN_SHARE : even;
}
inline int64_t cov_partials(int64_t N) { return N < 1 ? 0 : (N + cov_share(N) - 1) / cov_share(N); }
inline int cov_cpt(int64_t d) { return d <= 256 ? 1 : (d <= 512 ? 2 : 4); }

// One level of the fold over lane bit 5 / bit 4: a[l] + a[l ^ 32] lands in the lanes with the bit clear, b[l] + b[l ^ 32]
// in the lanes with it set (16: likewise).  v_permlane32_swap trades the upper half of its first operand for the lower
// half of its second, v_permlane16_swap the odd rows of 16 lanes for the even ones: two swaps and one addition per pair
// of values, no LDS and no select.
__device__ __forceinline__ double fold_swap32(double a, double b) {
    const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
    return __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
}
__device__ __forceinline__ double fold_swap16(double a, double b) {
    const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
    return __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
}

// A workgroup barrier that orders LDS traffic only: the next step's rows, loaded ahead into registers, stay in flight
// across it (__syncthreads would wait for them).
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <typename T, int CPT, bool WIDE>
__global__ __launch_bounds__(CV_T) void cov_partial_kernel(const T *__restrict__ X, int64_t N, int d, int64_t ld,
                                                           const double *__restrict__ mean,
                                                           const double *__restrict__ V, int p, int64_t share,
                                                           double *__restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) double cv_vs[];   // !WIDE: V transposed, [CV_P][CW]
    __shared__ double wsum[CV_T / 64][CV_NV];
    __shared__ double ysh[CV_NV];
    constexpr int CW = CV_T * CPT;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int chunk = WIDE ? (int)blockIdx.y : 0;
    const int nchunks = WIDE ? (d + CW - 1) / CW : 1;

    int col[CPT];
    bool ok[CPT];
    double mu[CPT];
#pragma unroll
    for (int u = 0; u < CPT; ++u) {
        col[u] = chunk * CW + t + CV_T * u;
        ok[u] = col[u] < d;
        mu[u] = (ok[u] && mean) ? mean[col[u]] : 0.0;
    }
    if (!WIDE) {
#pragma unroll
        for (int u = 0; u < CPT; ++u)
#pragma unroll
            for (int j = 0; j < CV_P; ++j)
                cv_vs[j * CW + t + CV_T * u] = (ok[u] && j < p) ? V[(size_t)col[u] * p + j] : 0.0;
        __syncthreads();
    }

    double Z[CPT][CV_P], cs[CPT];
#pragma unroll
    for (int u = 0; u < CPT; ++u) {
        cs[u] = 0.0;
#pragma unroll
        for (int j = 0; j < CV_P; ++j) Z[u][j] = 0.0;
    }

    const int64_t r_begin = (int64_t)blockIdx.x * share;
    const int64_t r_end = r_begin + share < N ? r_begin + share : N;
    // !WIDE: the rows of a step are loaded one step ahead
    T xr[CV_R][CPT];
    auto fetch = [&](int64_t r0) {
#pragma unroll
        for (int u = 0; u < CPT; ++u)
#pragma unroll
            for (int r = 0; r < CV_R; ++r)
                xr[r][u] = (ok[u] && r0 + r < r_end) ? X[(size_t)(r0 + r) * (size_t)ld + col[u]] : T(0);
    };
    if (!WIDE) fetch(r_begin);
    for (int64_t r0 = r_begin; r0 < r_end; r0 += CV_R) {
        double py[CV_NV], cown[CV_R][CPT];
#pragma unroll
        for (int v = 0; v < CV_NV; ++v) py[v] = 0.0;
#pragma unroll
        for (int r = 0; r < CV_R; ++r)
#pragma unroll
            for (int u = 0; u < CPT; ++u) cown[r][u] = 0.0;

        for (int cc = 0; cc < nchunks; ++cc) {
            const bool own = !WIDE || cc == chunk;
            double c[CV_R][CPT];
#pragma unroll
            for (int u = 0; u < CPT; ++u) {
                const int k = WIDE ? cc * CW + t + CV_T * u : col[u];
                const bool kok = k < d;
                const double m = WIDE ? ((kok && mean) ? mean[k] : 0.0) : mu[u];
#pragma unroll
                for (int r = 0; r < CV_R; ++r) {
                    if (WIDE) c[r][u] = (kok && r0 + r < r_end) ? widen(X[(size_t)(r0 + r) * (size_t)ld + k]) - m : 0.0;
                    else c[r][u] = (kok && r0 + r < r_end) ? widen(xr[r][u]) - m : 0.0;
                }
            }
            if (!WIDE && r0 + CV_R < r_end) fetch(r0 + CV_R);
#pragma unroll
            for (int u = 0; u < CPT; ++u) {
                double v[CV_P];
                if (WIDE) {
                    const int k = cc * CW + t + CV_T * u;
#pragma unroll
                    for (int j = 0; j < CV_P; ++j) v[j] = (k < d && j < p) ? V[(size_t)k * p + j] : 0.0;
                } else {
#pragma unroll
                    for (int j = 0; j < CV_P; ++j) v[j] = cv_vs[j * CW + t + CV_T * u];
                }
#pragma unroll
                for (int r = 0; r < CV_R; ++r)
#pragma unroll
                    for (int j = 0; j < CV_P; ++j) py[r * CV_P + j] += c[r][u] * v[j];
            }
            if (own) {
#pragma unroll
                for (int r = 0; r < CV_R; ++r)
#pragma unroll
                    for (int u = 0; u < CPT; ++u) cown[r][u] = c[r][u];
            }
        }

        // the wave's 32 partial sums: at the level of lane bit `mask` the two halves trade half of their values, so a
        // lane ends with ONE value summed over all 64 lanes -- value (lane >> 1) & 31 -- after 32 shuffles, not 192
#pragma unroll
        for (int i = 0; i < 16; ++i) py[i] = fold_swap32(py[i], py[i + 16]);
#pragma unroll
        for (int i = 0; i < 8; ++i) py[i] = fold_swap16(py[i], py[i + 8]);
#pragma unroll
        for (int s = 2; s < 5; ++s) {
            const int mask = 32 >> s, half = 16 >> s;
            const bool hi = (lane & mask) != 0;
#pragma unroll
            for (int i = 0; i < half; ++i) {
                const double send = hi ? py[i] : py[i + half];
                const double keep = hi ? py[i + half] : py[i];
                py[i] = keep + __shfl_xor(send, mask, 64);
            }
        }
        py[0] += __shfl_xor(py[0], 1, 64);
        if ((lane & 1) == 0) wsum[w][lane >> 1] = py[0];
        lds_barrier();
        if (t < CV_NV) ysh[t] = (wsum[0][t] + wsum[1][t]) + (wsum[2][t] + wsum[3][t]);
        lds_barrier();

#pragma unroll
        for (int r = 0; r < CV_R; ++r) {
#pragma unroll
            for (int j = 0; j < CV_P; ++j) {
                const double y = ysh[r * CV_P + j];
#pragma unroll
                for (int u = 0; u < CPT; ++u) Z[u][j] += cown[r][u] * y;
            }
#pragma unroll
            for (int u = 0; u < CPT; ++u) cs[u] += cown[r][u];
        }
    }

    double *mine = part + (size_t)blockIdx.x * (CV_P + 1) * (size_t)d;
#pragma unroll
    for (int u = 0; u < CPT; ++u) {
        if (!ok[u]) continue;
#pragma unroll
        for (int j = 0; j < CV_P; ++j) mine[(size_t)j * d + col[u]] = Z[u][j];
        mine[(size_t)CV_P * d + col[u]] = cs[u];
    }
}

// entry e = j d + l of the partials [nb][9][d], added in order: j < p -> Z[l, j], j == 8 -> s[l]
__global__ __launch_bounds__(256) void cov_final_kernel(const double *__restrict__ part, int64_t nb, int d, int p,
                                                        double *__restrict__ Z, double *__restrict__ colsum) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t stride = (int64_t)(CV_P + 1) * d;
    if (e >= stride) return;
    const int j = (int)(e / d), l = (int)(e % d);
    if (j >= p && j != CV_P) return;
    double s = 0.0;
    for (int64_t b = 0; b < nb; ++b) s += part[b * stride + e];
    if (j == CV_P) colsum[l] = s;
    else Z[(size_t)l * p + j] = s;
}

template <typename T, int CPT, bool WIDE>
static int cov_launch(const T *X, int64_t N, int d, int64_t ld, const double *mean, const double *V, int p, double *part,
                      hipStream_t s) {
    constexpr int CW = CV_T * CPT;
    const size_t lds = WIDE ? 0 : (size_t)CV_P * CW * sizeof(double);
    static bool attr = false;
    if (!attr && lds > 0) {
        DBGSOM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&cov_partial_kernel<T, CPT, WIDE>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr = true;
    }
    const dim3 grid((unsigned)cov_partials(N), WIDE ? (unsigned)((d + CW - 1) / CW) : 1u);
    hipLaunchKernelGGL((cov_partial_kernel<T, CPT, WIDE>), grid, dim3(CV_T), lds, s, X, N, d, ld, mean, V, p, cov_share(N),
                       part);
    return launch_status("cov_partial_kernel");
}

template <typename T>
static int cov_dispatch(const T *X, int64_t N, int d, int64_t ld, const double *mean, const double *V, int p, double *part,
                        hipStream_t s) {
    if (d > CV_T * CV_MAX_CPT) return cov_launch<T, CV_MAX_CPT, true>(X, N, d, ld, mean, V, p, part, s);
    switch (cov_cpt(d)) {
        case 1: return cov_launch<T, 1, false>(X, N, d, ld, mean, V, p, part, s);
        case 2: return cov_launch<T, 2, false>(X, N, d, ld, mean, V, p, part, s);
        default: return cov_launch<T, 4, false>(X, N, d, ld, mean, V, p, part, s);
    }
}

}  // namespace dbgsom

using namespace dbgsom;

extern "C" {

size_t dbgsom_covariance_apply_workspace_bytes(int64_t N, int64_t d, int p) {
    if (N < 1 || d < 1 || p < 1 || p > CV_P) return 0;
    return (size_t)cov_partials(N) * (CV_P + 1) * (size_t)d * sizeof(double);
}

int dbgsom_covariance_apply(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *mean_dev,
                            const double *V_dev, int p, double *Z_dev, double *colsum_dev, void *workspace_dev,
                            size_t workspace_bytes, void *stream) {
    DBGSOM_REQUIRE(x_dtype == DBGSOM_F32 || x_dtype == DBGSOM_F64, "float32 / float64 rows only (x_dtype)");
    DBGSOM_REQUIRE(p >= 1 && p <= CV_P, "p must be 1 .. DBGSOM_MAX_DIRECTIONS");
    DBGSOM_REQUIRE(N >= 0 && d >= 1 && d <= (1 << 30) && ldx >= d, "bad shape (N >= 0, 1 <= d <= 2^30, ldx >= d)");
    DBGSOM_REQUIRE(V_dev && Z_dev && colsum_dev, "null pointer");
    DBGSOM_REQUIRE(N == 0 || X_dev, "null input");
    const size_t need = dbgsom_covariance_apply_workspace_bytes(N, d, p);
    if (workspace_bytes < need || (need > 0 && !workspace_dev)) {
        set_error("dbgsom_covariance_apply: workspace too small (%zu bytes given, %zu needed)", workspace_bytes, need);
        return DBGSOM_ENOMEM;
    }
    DBGSOM_REQUIRE(is_aligned(workspace_dev, 16), "workspace_dev must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (N == 0) {
        DBGSOM_HIP_CHECK(hipMemsetAsync(Z_dev, 0, (size_t)d * p * sizeof(double), s));
        DBGSOM_HIP_CHECK(hipMemsetAsync(colsum_dev, 0, (size_t)d * sizeof(double), s));
        return DBGSOM_OK;
    }
    double *part = (double *)workspace_dev;
    int rc = x_dtype == DBGSOM_F32 ? cov_dispatch((const float *)X_dev, N, (int)d, ldx, mean_dev, V_dev, p, part, s)
                                   : cov_dispatch((const double *)X_dev, N, (int)d, ldx, mean_dev, V_dev, p, part, s);
    if (rc != DBGSOM_OK) return rc;
    const int64_t entries = (int64_t)(CV_P + 1) * d;
    hipLaunchKernelGGL(cov_final_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, s, part, cov_partials(N),
                       (int)d, p, Z_dev, colsum_dev);
    return launch_status("cov_final_kernel");
}

}  // extern "C"
