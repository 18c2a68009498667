// The direct-form kernels in which the lanes own prototypes: the searches over CSR rows (csr.hip), over rows with
// missing entries (masked.hip) and under metric="manhattan" (manhattan.hip), and the siblings of the last two that
// store every distance.
//
// Layout: the lanes of a workgroup own prototypes and read Wt, the transposed float64 prototypes (d x ldwt, zeros
// behind column M), so one feature is one coalesced 512-byte read per wavefront, shared by the R rows the workgroup
// walks as R independent chains per lane.  The rows' entries are the same for every lane: they arrive by scalar loads.
// Winners are the lexicographic minimum on (value, index) through Best<K>, as everywhere in this library.
//
// A form is a Term (what one entry adds to a pair's chain) and a Finish (what is written from a chain's end).  The
// dense forms share the step and the store kernel below; direct_bmu_kernel is the L1 search, and masked_bmu_kernel
// (masked.hip) the same statements with its own argument list.  bmu_csr_kernel walks stored entries and keeps its own
// body.  All three searches end in the one winners' tail.
#pragma once
#include "bmu_common.h"

namespace dbgsom {

constexpr int MT = 256;    // threads per workgroup = prototypes per block of the search
constexpr int MR = 16;     // rows per workgroup (independent chains per lane) when there are many rows
constexpr int MU = 4;      // features per step of the inner loop (one scalar load per row and step)
constexpr int MRS = 4;     // ... when there are few: more workgroups
constexpr int64_t MASKED_FEW_ROWS = 8192;

// NaN test of a wave-uniform value on the scalar unit: (|hi| | (lo != 0)) > 0x7ff00000.  Written as a comparison
// the compiler moves "lo != 0" to the vector unit (three more vector instructions per entry); s_min_u32 keeps it an
// integer.
__device__ __forceinline__ bool nan_bits_uniform(double x) {
    const uint32_t hi = (uint32_t)__double2hiint(x) & 0x7fffffffu, lo = (uint32_t)__double2loint(x);
    uint32_t lo_nz;
    asm("s_min_u32 %0, %1, 1" : "=s"(lo_nz) : "s"(lo) : "scc");
    return (hi | lo_nz) > 0x7ff00000u;
}

// ---- terms: entry x of a row against entry w of this lane's prototype -------------------------------------
// rows with missing entries: t = x - w; acc = fma(t, t, acc) over the observed entries.  The skip of a missing entry
// has to stay a branch of the scalar unit: as a select it would cost two more vector instructions per entry than the
// arithmetic itself (the empty asm keeps the compiler from turning it into one).
struct SquaredObservedTerm {
    static __device__ __forceinline__ void add(double x, double w, double &acc) {
        if (!nan_bits_uniform(x)) {
            double t = x - w;
            asm volatile("" : "+v"(t));
            acc = fma(t, t, acc);
        }
    }
};
// metric="manhattan": acc = acc + |x - w| (two v_add_f64: the negation and the absolute value are source modifiers)
struct AbsTerm {
    static __device__ __forceinline__ void add(double x, double w, double &acc) { acc = acc + fabs(x - w); }
};

// ---- finishes: row(i, d) is what a finish needs of row i of d features, value(v, row) what is written for a chain
// that ended at v ---------------------------------------------------------------------------------------------
struct PlainFinish {   // the value itself
    __device__ __forceinline__ double row(int64_t, int) const { return 0.0; }
    __device__ __forceinline__ double value(double v, double) const { return v; }
};
struct RootFinish {    // its square root, optionally rounded to float32 (the epilogue of bmu_kernel)
    int round_f32;
    __device__ __forceinline__ double row(int64_t, int) const { return 0.0; }
    __device__ __forceinline__ double value(double v, double) const {
        const double dv = sqrt(v);
        return round_f32 ? (double)(float)dv : dv;
    }
};
template <bool SQ>     // rows with missing entries: scaled by d / n_obs; SQ: without the square root
struct ObservedFinish {
    const int32_t *nobs;
    // (no observed entry: 0 * inf, the distance is NaN)
    __device__ __forceinline__ double row(int64_t i, int d) const { return (double)d / (double)nobs[i]; }
    __device__ __forceinline__ double value(double v, double scale) const { return SQ ? v * scale : sqrt(v * scale); }
};

// ---- U features of R rows against this lane's prototype: acc[r] goes on along its chain, k ascending ------
// (uniform: the same entries for every lane; the next row's load is in flight while this row is worked on)
template <typename Term, int R, int U>
__device__ __forceinline__ void dense_step(const double *__restrict__ xb, const uint32_t (&off)[R], int e,
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
        for (int u = 0; u < U; ++u) Term::add(x[u], w[u], acc[r]);
    }
}

// ---- the winners' tail of a workgroup of MT lanes that walked rows i0 .. i0 + nrows - 1 ------------------
// best: the Best<K> best[R] of each lane.  The lanes of a wavefront, then the wavefronts, hold different prototypes of
// the same rows: 64-lane merges, the wavefronts' lists through LDS, then one lane per row writes idx (-1: no pair was
// below +inf, Best::push) and dist = fin.value(v, fin.row(i, d)).
// A macro and not a function, so that the kernels stay the ones they were: as a function the tail's stack objects are
// laid out in front of the caller's lists (K = 2: 16 bytes more scratch per lane) and the K = 1 merges compile to
// exec-masked moves instead of selects (16 instructions more per row).
#define DBGSOM_STORE_WINNERS(K, R, best, i0, nrows, d, fin, idx_out, dist_out)                                      \
    do {                                                                                                            \
        __shared__ double mv_[MT / 64][R][K];                                                                       \
        __shared__ int mj_[MT / 64][R][K];                                                                          \
        const int tid_ = threadIdx.x, lane_ = tid_ & 63, wave_ = tid_ >> 6;                                         \
        _Pragma("unroll") for (int r = 0; r < R; ++r) {                                                             \
            _Pragma("unroll") for (int m = 1; m < 64; m <<= 1) {                                                    \
                double ov[K];                                                                                       \
                int oj[K];                                                                                          \
                _Pragma("unroll") for (int t = 0; t < K; ++t) {                                                     \
                    ov[t] = __shfl_xor(best[r].v[t], m, 64);                                                        \
                    oj[t] = __shfl_xor(best[r].j[t], m, 64);                                                        \
                }                                                                                                   \
                best[r].merge(ov, oj);                                                                              \
            }                                                                                                       \
            if (lane_ == 0) {                                                                                       \
                _Pragma("unroll") for (int t = 0; t < K; ++t) {                                                     \
                    mv_[wave_][r][t] = best[r].v[t];                                                                \
                    mj_[wave_][r][t] = best[r].j[t];                                                                \
                }                                                                                                   \
            }                                                                                                       \
        }                                                                                                           \
        __syncthreads();                                                                                            \
        if (tid_ < nrows) {                                                                                         \
            Best<K> b;                                                                                              \
            _Pragma("unroll") for (int t = 0; t < K; ++t) { b.v[t] = mv_[0][tid_][t]; b.j[t] = mj_[0][tid_][t]; }   \
            _Pragma("unroll") for (int w = 1; w < MT / 64; ++w) {                                                   \
                double ov[K];                                                                                       \
                int oj[K];                                                                                          \
                _Pragma("unroll") for (int t = 0; t < K; ++t) { ov[t] = mv_[w][tid_][t]; oj[t] = mj_[w][tid_][t]; } \
                b.merge(ov, oj);                                                                                    \
            }                                                                                                       \
            const int64_t i = i0 + tid_;                                                                            \
            const double row = fin.row(i, d);                                                                       \
            _Pragma("unroll") for (int t = 0; t < K; ++t) {                                                         \
                idx_out[i * K + t] = (b.j[t] == 0x7fffffff) ? (int64_t)-1 : (int64_t)b.j[t];                        \
                dist_out[i * K + t] = fin.value(b.v[t], row);                                                       \
            }                                                                                                       \
        }                                                                                                           \
    } while (0)

// ---- search: the K nearest prototypes of every row ------------------------------------------------------
// (metric="manhattan".  The search over rows with missing entries, masked_bmu_kernel of masked.hip, is this kernel with
//  n_obs where it always was in the argument list: merged into this one it measured 0.2 % slower at 50 % missing.)
template <typename Term, typename Finish, int K, int R>
__global__ __launch_bounds__(MT) void direct_bmu_kernel(const double *__restrict__ X, int64_t N, int d, int64_t ldx,
                                                        const double *__restrict__ Wt, int64_t ldwt, int M,
                                                        int64_t *__restrict__ idx_out, double *__restrict__ dist_out,
                                                        Finish fin) {
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
        for (; e + MU <= d; e += MU) dense_step<Term, R, MU>(xb, off, e, wcol, ldwt, acc);
        for (; e < d; ++e) dense_step<Term, R, 1>(xb, off, e, wcol, ldwt, acc);
        if (j < M) {
#pragma unroll
            for (int r = 0; r < R; ++r) best[r].push(acc[r], j);
        }
    }
    DBGSOM_STORE_WINNERS(K, R, best, i0, nrows, d, fin, idx_out, dist_out);
}

// ---- the same loop, every (row, prototype) stored -------------------------------------------------------
// The lanes own prototypes, so the 256 distances of a row and prototype block are contiguous: one 8-byte store per
// lane is a coalesced 512-byte store per wavefront whatever the alignment of `out` and ldo.  CACHED: the slab of the
// selection is read back at once (ordinary stores); the full matrix is never read again here (non-temporal stores).
// SPLIT: the prototype blocks are divided over blockIdx.y (a pair's chain does not depend on the workgroup that runs
// it).  A compile-time property, because the stride costs the 16-row form of the rows with missing entries 26
// registers and a wave per SIMD: that form is launched with gridDim.y = 1 and compiled without it.
template <typename Term, typename Finish, int R, bool CACHED, bool SPLIT>
__global__ __launch_bounds__(MT) void direct_dist_kernel(const double *__restrict__ X, int64_t N, int d, int64_t ldx,
                                                         const double *__restrict__ Wt, int64_t ldwt, int M,
                                                         double *__restrict__ out, int64_t ldo, Finish fin) {
    const int tid = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * R;
    const int nrows = (int)min((int64_t)R, N - i0);
    const double *__restrict__ xb = X + i0 * ldx;
    uint32_t off[R];   // (rows behind the last one repeat it: computed, never written; R ldx < 2^32 is required)
    double row[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        off[r] = (uint32_t)min(r, nrows - 1) * (uint32_t)ldx;
        row[r] = fin.row(i0 + min(r, nrows - 1), d);
    }
    for (int jb = SPLIT ? (int)blockIdx.y * MT : 0; jb < M; jb += SPLIT ? (int)gridDim.y * MT : MT) {
        const int j = jb + tid;            // (j < ldwt: the columns behind M hold zeros)
        const double *__restrict__ wcol = Wt + j;
        double acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0.0;
        int e = 0;
        for (; e + MU <= d; e += MU) dense_step<Term, R, MU>(xb, off, e, wcol, ldwt, acc);
        for (; e < d; ++e) dense_step<Term, R, 1>(xb, off, e, wcol, ldwt, acc);
        if (j < M) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (r < nrows) {
                    double *p = out + (i0 + r) * ldo + j;
                    if constexpr (CACHED) *p = fin.value(acc[r], row[r]);
                    else __builtin_nontemporal_store(fin.value(acc[r], row[r]), p);
                }
            }
        }
    }
}

// ---- launches: few rows -> MRS rows per workgroup, many -> MR; Wt is launch_transpose_weights' (ldwt = csr_wt_ld(M)) --
// a search of N rows: Family<K, R>::kernel over (few rows / many rows) x (k = 1 / 2), `args` its arguments
template <template <int, int> class Family, typename... Args>
inline void launch_bmu_rows(int64_t N, int k, hipStream_t s, Args... args) {
    const bool few = N < MASKED_FEW_ROWS;
    const dim3 grid((unsigned)(few ? (N + MRS - 1) / MRS : (N + MR - 1) / MR));
    auto *kernel = few ? (k == 1 ? Family<1, MRS>::kernel : Family<2, MRS>::kernel)
                       : (k == 1 ? Family<1, MR>::kernel : Family<2, MR>::kernel);
    hipLaunchKernelGGL(kernel, grid, dim3(MT), 0, s, args...);
}

// gy: the shares the prototype blocks are divided into (SPLIT forms; 1 otherwise)
template <typename Term, typename Finish, bool CACHED, bool SPLIT>
inline void launch_direct_dist(const double *X64, int64_t N, int64_t d, int64_t ld64, const double *Wt, int64_t M,
                               double *out, int64_t ldo, Finish fin, unsigned gy, hipStream_t s) {
    const int64_t ldwt = csr_wt_ld(M);
    const bool few = N < MASKED_FEW_ROWS;
    const dim3 grid((unsigned)(few ? (N + MRS - 1) / MRS : (N + MR - 1) / MR), SPLIT ? gy : 1u);
    auto *kernel = few ? direct_dist_kernel<Term, Finish, MRS, CACHED, SPLIT> : direct_dist_kernel<Term, Finish, MR, CACHED, SPLIT>;
    hipLaunchKernelGGL(kernel, grid, dim3(MT), 0, s, X64, N, (int)d, ld64, Wt, ldwt, (int)M, out, ldo, fin);
}

}  // namespace dbgsom
