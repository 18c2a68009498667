// Non-negative LARS-lasso sparse coding of query rows over the prototypes on gfx950 (MI355X):
// the path of BaseSom.transform and SomClassifier.predict_proba (reference dbgsom/BaseSom.py:241-268,
// SomClassifier.py:178-220), i.e. scikit-learn's
//     SparseCoder(dictionary=normalize(W), transform_algorithm="lasso_lars", positive_code=True,
//                 transform_alpha=0).transform(normalize(X))
// which is, per query row x:  lars_path_gram(Xy = Wn xn, Gram = Wn Wn^T, n_samples = d,
// method="lasso", positive=True, alpha_min=0)  (sklearn/linear_model/_least_angle.py,
// _lars_path_solver, the Gram branch without the path).
//
// Stages (DESIGN.md "Sparse coding"):
//   1. row normalisation: W in float64; float32 queries in float32 (sklearn's normalize keeps the
//      dtype), widened to float64 afterwards.
//   2. G = Wn Wn^T and Cov = Xn Wn^T on the float64 matrix cores (v_mfma_f64_16x16x4_f64).
//   3. LARS: one 64-lane workgroup (one wave) per query row.  Per-prototype state (Cov, the
//      prototype's POSITION in sklearn's permuted `indices`) lives in per-row global scratch in the
//      prototypes' original order, so G rows are read coalesced and sklearn's argmax tie rule is
//      "largest Cov, then smallest position".  The active set (its Cholesky factor L, packed with
//      one spare slot per row for the Givens downdate, the coefficients) lives in LDS up to a
//      compile-time cap; a row whose active set outgrows the (runtime) cap is listed and solved
//      again from the start by the overflow pass, which keeps the same state in global slots.
//   4. epilogue: the code row, and/or sum_a coef_a P[a, :] normalised (predict_proba).
// Every row is finished on the device; there is no host fallback.
#include <float.h>
#include <math.h>

#include <algorithm>

#include "common.h"

namespace dbgsom {

namespace {

typedef double d4_t __attribute__((ext_vector_type(4)));

constexpr int SC_CAP = 64;                                // fast-path active-set cap (LDS)
constexpr int SC_GT = 64;                                 // GEMM output tile (rows and columns)
constexpr int SC_KT = 16;                                 // GEMM k tile
constexpr int SC_LS = SC_KT + 2;                          // LDS row stride of a GEMM tile (doubles)
constexpr double TINY32 = 1.1754943508222875e-38;         // np.finfo(np.float32).tiny
constexpr double EPS32 = 1.1920928955078125e-07;          // np.finfo(np.float32).eps
constexpr double EPS64 = 2.220446049250313e-16;           // np.finfo(float).eps

__host__ __device__ constexpr int64_t lpk_size(int64_t cap) { return cap * (cap + 3) / 2; }
// row i of the packed factor starts here and has i + 2 slots (one spare for the downdate's shift)
__device__ __forceinline__ int lrow(int i) { return i * (i + 3) / 2; }

// ------------------------------------------------------------------------------------------------
// 1. row normalisation (sklearn.preprocessing.normalize, norm="l2"): a norm below 10 eps of the dtype is
//    taken as 1 (sklearn's _handle_zeros_in_scale), so zero and near-zero rows stay as they are
// ------------------------------------------------------------------------------------------------
template <typename XT>
__global__ __launch_bounds__(64) void sc_normalize_kernel(const XT *__restrict__ X, int64_t N, int d, int64_t ldx,
                                                          double *__restrict__ out, int64_t ldo) {
    const int lane = threadIdx.x;
    const int64_t i = blockIdx.x;
    if (i >= N) return;
    const XT *x = X + i * ldx;
    double *o = out + i * ldo;
    if constexpr (sizeof(XT) == 4) {
        // float32 arithmetic throughout, as sklearn does for a float32 array
        float s = 0.0f;
        for (int k = lane; k < d; k += 64) s += x[k] * x[k];
        for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
        float nrm = sqrtf(s);
        if (nrm < 10.0f * FLT_EPSILON) nrm = 1.0f;
        for (int k = lane; k < d; k += 64) o[k] = (double)(x[k] / nrm);
    } else {
        double s = 0.0;
        for (int k = lane; k < d; k += 64) s += (double)x[k] * (double)x[k];
        for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
        double nrm = sqrt(s);
        if (nrm < 10.0 * DBL_EPSILON) nrm = 1.0;
        for (int k = lane; k < d; k += 64) o[k] = (double)x[k] / nrm;
    }
}

// ------------------------------------------------------------------------------------------------
// 2. C[n x m] = A[n x K] B[m x K]^T in float64 on the matrix cores.  256 threads = 2 x 2 waves, a
//    64 x 64 output tile, each wave 2 x 2 tiles of v_mfma_f64_16x16x4_f64 (operand layout of
//    bmu.hip: a tile row is lane & 15, the k slot lane >> 4; the accumulator's element r of lane l is
//    row 4 r + (l >> 4), column l & 15).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sc_gemm_nt_kernel(const double *__restrict__ A, int64_t n, int64_t lda,
                                                         const double *__restrict__ B, int64_t m, int64_t ldb, int K,
                                                         double *__restrict__ C, int64_t ldc) {
    __shared__ __attribute__((aligned(16))) double as[SC_GT * SC_LS];
    __shared__ __attribute__((aligned(16))) double bs[SC_GT * SC_LS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1;
    const int lr = lane & 15, lq = lane >> 4;
    const int64_t i0 = (int64_t)blockIdx.x * SC_GT, j0 = (int64_t)blockIdx.y * SC_GT;  // row tiles on grid x
    const int srow = tid >> 2, sk = (tid & 3) * 4;  // staging: 4 threads per tile row, 4 values each
    d4_t acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = d4_t{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < K; k0 += SC_KT) {
        const int64_t ia = i0 + srow, jb = j0 + srow;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int k = k0 + sk + e;
            as[srow * SC_LS + sk + e] = (ia < n && k < K) ? A[ia * lda + k] : 0.0;
            bs[srow * SC_LS + sk + e] = (jb < m && k < K) ? B[jb * ldb + k] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < SC_KT / 4; ++ks) {
            double a[2], b[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                a[u] = as[(wi * 32 + u * 16 + lr) * SC_LS + ks * 4 + lq];
                b[u] = bs[(wj * 32 + u * 16 + lr) * SC_LS + ks * 4 + lq];
            }
#pragma unroll
            for (int ta = 0; ta < 2; ++ta)
#pragma unroll
                for (int tb = 0; tb < 2; ++tb)
                    acc[ta][tb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ta], b[tb], acc[ta][tb], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int ta = 0; ta < 2; ++ta)
#pragma unroll
        for (int tb = 0; tb < 2; ++tb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t i = i0 + wi * 32 + ta * 16 + 4 * r + lq;
                const int64_t j = j0 + wj * 32 + tb * 16 + lr;
                if (i < n && j < m) C[i * ldc + j] = acc[ta][tb][r];
            }
}

int launch_gemm_nt(const double *A, int64_t n, int64_t lda, const double *B, int64_t m, int64_t ldb, int64_t K,
                   double *C, int64_t ldc, hipStream_t s) {
    if (n == 0 || m == 0) return DBGSOM_OK;
    if ((m + SC_GT - 1) / SC_GT > 65535) {
        set_error("sparse code: %lld prototypes exceed the GEMM grid", (long long)m);
        return DBGSOM_EINVAL;
    }
    hipLaunchKernelGGL(sc_gemm_nt_kernel, dim3((unsigned)((n + SC_GT - 1) / SC_GT), (unsigned)((m + SC_GT - 1) / SC_GT)),
                       dim3(256), 0, s, A, n, lda, B, m, ldb, (int)K, C, ldc);
    return launch_status("sc_gemm_nt_kernel");
}

// ------------------------------------------------------------------------------------------------
// 3. LARS, one wave per query row
// ------------------------------------------------------------------------------------------------
struct LarsArgs {
    const double *G;       // M x M, Wn Wn^T
    const double *cov0;    // rows x M, Xn Wn^T (sklearn's Cov_copy)
    double *cov;           // rows x M working Cov (original prototype order)
    double *ced;           // rows x M corr_eq_dir of the running iteration
    int32_t *pos;          // rows x M position of every prototype in sklearn's `indices`
    int M, d, max_iter, cap;
    int64_t rows;
    const double *P;       // M x C class frequencies (nullable)
    int C;
    double *code;          // rows x M (nullable)
    double *proba;         // rows x C (nullable)
    unsigned long long *counts;  // DBGSOM_SC_N_COUNTS
    int32_t *ovf_list;     // rows whose active set outgrew the fast path's cap
    uint32_t *ovf_n;
    double *slot_ws;       // overflow passes: per-workgroup slot (factor + active-set vectors)
};

// the active-set state of one row: in LDS (fast path) or in a global slot (overflow pass)
struct ActiveSet {
    double *L;      // packed lower factor, lpk_size(cap)
    double *coef;   // coefficient of active slot k (original feature act[k])
    double *ls;     // least_squares
    double *y;      // scratch vector
    double *dg;     // diagonal of the retry factor (non-finite AA)
    double *va0, *va1;  // coefficient vectors of the last two assignments (sklearn's coef / prev_coef)
    int *fa0, *fa1;     // ... their features
    __device__ double *va(int w) const { return w ? va1 : va0; }
    __device__ int *fa(int w) const { return w ? fa1 : fa0; }
    int *act;       // active features in position order (== sklearn's `active`)
};

__device__ __forceinline__ void wave_sync() { __syncthreads(); }  // one wave per workgroup

__device__ __forceinline__ double wave_sum(double v) {
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ double wave_min(double v) {
    for (int m = 32; m >= 1; m >>= 1) v = fmin(v, __shfl_xor(v, m, 64));
    return v;
}

// y <- L^{-1} y (forward substitution, column order of BLAS dtrsv "L", "N"); n <= cap; diag from `dg`
// when given
__device__ void fwd_solve(const double *L, double *y, int n, const double *dg, int lane) {
    for (int j = 0; j < n; ++j) {
        const double yj = y[j] / (dg ? dg[j] : L[lrow(j) + j]);
        wave_sync();
        if (lane == 0) y[j] = yj;
        for (int i = j + 1 + lane; i < n; i += 64) y[i] -= L[lrow(i) + j] * yj;
        wave_sync();
    }
}
// y <- L^{-T} y (back substitution, column order)
__device__ void bwd_solve(const double *L, double *y, int n, const double *dg, int lane) {
    for (int j = n - 1; j >= 0; --j) {
        const double yj = y[j] / (dg ? dg[j] : L[lrow(j) + j]);
        wave_sync();
        if (lane == 0) y[j] = yj;
        for (int i = lane; i < j; i += 64) y[i] -= L[lrow(j) + i] * yj;
        wave_sync();
    }
}

// sklearn.utils.arrayfuncs.cholesky_delete on the n x n factor: drop row `go`, shift the rows below
// up, restore the lower-triangular form with Givens rotations (BLAS drotg / drot)
__device__ void cholesky_delete(double *L, int n, int go, int lane) {
    for (int i = go; i < n - 1; ++i) {  // row i <- row i + 1 (i + 2 values; ranges do not overlap)
        for (int k = lane; k < i + 2; k += 64) L[lrow(i) + k] = L[lrow(i + 1) + k];
        wave_sync();
    }
    for (int i = go; i < n - 1; ++i) {
        const double a = L[lrow(i) + i], b = L[lrow(i) + i + 1];
        double c, s, r;
        const double scale = fabs(a) + fabs(b);
        if (scale == 0.0) {
            c = 1.0; s = 0.0; r = 0.0;
        } else {
            const double roe = fabs(a) > fabs(b) ? a : b;
            r = scale * sqrt((a / scale) * (a / scale) + (b / scale) * (b / scale));
            if (roe < 0.0) r = -r;
            c = a / r;
            s = b / r;
        }
        if (r < 0.0) { r = fabs(r); c = -c; s = -s; }
        wave_sync();
        if (lane == 0) { L[lrow(i) + i] = r; L[lrow(i) + i + 1] = 0.0; }
        for (int j = i + 1 + lane; j < n - 1; j += 64) {
            const double x = L[lrow(j) + i], y = L[lrow(j) + i + 1];
            L[lrow(j) + i] = c * x + s * y;
            L[lrow(j) + i + 1] = c * y - s * x;
        }
        wave_sync();
    }
}

// the order of DBGSOM_SC_COUNTS in include/dbgsom_hip.h
enum { CNT_SAMPLES = 0, CNT_ITERS, CNT_ITER_MAX, CNT_DROPS, CNT_DEGENERATE, CNT_EARLY, CNT_AA_RETRY, CNT_OVERFLOW,
       CNT_ACTIVE_MAX, CNT_MULTI_DROP, CNT_G_ROWS };
static_assert(CNT_G_ROWS + 1 == DBGSOM_SC_COUNTS, "counter layout");

// solves row `row`; returns false when the active set outgrew `cap` (fast path: the row is listed)
__device__ bool lars_row(const LarsArgs &a, int64_t row, ActiveSet &st, int cap, int lane) {
    const int M = a.M;
    const double *G = a.G;
    const double *cov0 = a.cov0 + row * (int64_t)M;
    double *cov = a.cov + row * (int64_t)M;
    double *ced = a.ced + row * (int64_t)M;
    int32_t *pos = a.pos + row * (int64_t)M;
    for (int f = lane; f < M; f += 64) { cov[f] = cov0[f]; pos[f] = f; }
    int na = 0, n_iter = 0, cur = 0, ncur = 0, nprev = 0;
    bool drop = false, interp = false;
    double prev_alpha = 0.0, ss = 0.0;
    unsigned long long n_drop = 0, n_deg = 0, n_early = 0, n_retry = 0, n_multi = 0, g_rows = 0;
    int max_act = 0;
    wave_sync();
    for (;;) {
        // argmax of Cov over the inactive prototypes; ties -> smallest position
        double best = -INFINITY;
        int bpos = 0x7fffffff, bf = -1, fm = -1;
        for (int f = lane; f < M; f += 64) {
            const int p = pos[f];
            if (p >= na) {
                const double v = cov[f];
                if (v > best || (v == best && p < bpos) || (bf < 0 && v != v)) { best = v; bpos = p; bf = f; }
                if (p == na) fm = f;
            }
        }
        for (int m = 32; m >= 1; m >>= 1) {
            const double ob = __shfl_xor(best, m, 64);
            const int op = __shfl_xor(bpos, m, 64), of = __shfl_xor(bf, m, 64), om = __shfl_xor(fm, m, 64);
            if (of >= 0 && (bf < 0 || ob > best || (ob == best && op < bpos))) { best = ob; bpos = op; bf = of; }
            fm = max(fm, om);
        }
        const double C = (na < M) ? best : 0.0;
        const double alpha = C / (double)a.d;
        if (alpha <= 0.0 + EPS32) {  // early stopping at alpha_min = 0
            if (fabs(alpha) > EPS32 && n_iter > 0) { ss = prev_alpha / (prev_alpha - alpha); interp = true; }
            break;
        }
        if (n_iter >= a.max_iter || na >= M) break;
        if (!drop) {
            if (bf < 0) break;  // (no comparable Cov left: NaN input)
            const int fc = bf;
            if (fm < 0) fm = fc;
            if (na >= cap) return false;
            // new row of the factor: solve L y = G[fc, active]
            for (int k = lane; k < na; k += 64) st.y[k] = G[(int64_t)fc * M + st.act[k]];
            wave_sync();
            fwd_solve(st.L, st.y, na, nullptr, lane);
            double v = 0.0;
            for (int k = lane; k < na; k += 64) v += st.y[k] * st.y[k];
            v = wave_sum(v);
            const double cdiag = G[(int64_t)fc * M + fc];
            const double diag = fmax(sqrt(fabs(cdiag - v)), EPS64);
            const int pc = pos[fc];
            wave_sync();
            if (diag < 1e-7) {
                // degenerate regressor: sklearn zeroes Cov at the swapped-in slot and swaps the Cov values
                // back, but not `indices`: fc takes position na with fm's Cov, fm takes fc's old position
                // with Cov 0
                ++n_deg;
                if (lane == 0) {
                    const double vm = cov[fm];
                    cov[fc] = vm;
                    cov[fm] = 0.0;
                    pos[fm] = pc;
                    pos[fc] = na;
                }
                wave_sync();
                continue;
            }
            for (int k = lane; k < na; k += 64) st.L[lrow(na) + k] = st.y[k];
            if (lane == 0) {
                st.L[lrow(na) + na] = diag;
                st.act[na] = fc;
                st.coef[na] = 0.0;
                pos[fm] = pc;
                pos[fc] = na;
            }
            ++na;
            max_act = max(max_act, na);
            wave_sync();
        }
        if (n_iter > 0 && prev_alpha < alpha) { ++n_early; break; }  // lasso: alpha no longer decreases
        // least_squares: L L^T ls = 1 (potrs), AA = 1 / sqrt(sum ls)
        for (int k = lane; k < na; k += 64) st.ls[k] = 1.0;
        wave_sync();
        fwd_solve(st.L, st.ls, na, nullptr, lane);
        bwd_solve(st.L, st.ls, na, nullptr, lane);
        double AA;
        if (na == 1 && st.ls[0] == 0.0) {
            wave_sync();
            if (lane == 0) st.ls[0] = 1.0;
            AA = 1.0;
        } else {
            double sl = 0.0;
            for (int k = lane; k < na; k += 64) sl += st.ls[k];
            sl = wave_sum(sl);
            AA = 1.0 / sqrt(sl);
            if (!isfinite(AA)) {
                ++n_retry;
                for (int k = lane; k < na; k += 64) st.dg[k] = st.L[lrow(k) + k];
                for (int i = 0; !isfinite(AA); ++i) {
                    wave_sync();
                    for (int k = lane; k < na; k += 64) { st.dg[k] += ldexp(1.0, i) * EPS64; st.ls[k] = 1.0; }
                    wave_sync();
                    fwd_solve(st.L, st.ls, na, st.dg, lane);
                    bwd_solve(st.L, st.ls, na, st.dg, lane);
                    double t = 0.0;
                    for (int k = lane; k < na; k += 64) t += st.ls[k];
                    t = fmax(wave_sum(t), EPS64);
                    AA = 1.0 / sqrt(t);
                }
            }
            wave_sync();
            for (int k = lane; k < na; k += 64) st.ls[k] *= AA;
        }
        wave_sync();
        // corr_eq_dir = G[active, inactive]^T ls, rounded to 15 decimals; g1 = min_pos((C - Cov) / (AA - ced))
        g_rows += (unsigned long long)na;
        double g1 = DBL_MAX;
        for (int f = lane; f < M; f += 64) {
            if (pos[f] < na) continue;
            double e = 0.0;
            for (int k = 0; k < na; ++k) e += G[(int64_t)st.act[k] * M + f] * st.ls[k];
            e = rint(e * 1e15) / 1e15;
            ced[f] = e;
            const double q = (C - cov[f]) / (AA - e + TINY32);
            if (q > 0.0 && q < g1) g1 = q;
        }
        g1 = wave_min(g1);
        double gamma = fmin(g1, C / AA);
        // drops: z = -coef / (ls + tiny32)
        double zpos = DBL_MAX;
        for (int k = lane; k < na; k += 64) {
            const double z = -st.coef[k] / (st.ls[k] + TINY32);
            st.y[k] = z;  // kept for the drop test below
            if (z > 0.0 && z < zpos) zpos = z;
        }
        zpos = wave_min(zpos);
        drop = zpos < gamma;
        if (drop) gamma = zpos;
        ++n_iter;
        // coef[active] = prev_coef[active] + gamma ls  (the vector of the previous assignment is kept: the
        // final interpolation and a dropped prototype's Cov read it)
        cur ^= 1;
        nprev = ncur;
        ncur = na;
        for (int k = lane; k < na; k += 64) {
            const double c = st.coef[k] + gamma * st.ls[k];
            st.coef[k] = c;
            st.va(cur)[k] = c;
            st.fa(cur)[k] = st.act[k];
        }
        prev_alpha = alpha;
        for (int f = lane; f < M; f += 64)
            if (pos[f] >= na) cov[f] -= gamma * ced[f];
        wave_sync();
        if (drop) {
            // every active slot with z == z_pos, highest slot first (more than one: counted)
            const unsigned long long drops_before = n_drop;
            for (int kk = na - 1; kk >= 0; --kk) {
                if (st.y[kk] != zpos) continue;  // (slots below kk have not moved)
                const int fd = st.act[kk];
                cholesky_delete(st.L, na, kk, lane);
                // Cov of the dropped prototype from the unpermuted Cov_copy - Gram_copy coef
                double t = 0.0;
                for (int j = lane; j < ncur; j += 64) t += G[(int64_t)fd * M + st.fa(cur)[j]] * st.va(cur)[j];
                t = wave_sum(t);
                wave_sync();
                if (lane == 0) {
                    for (int k = kk; k < na - 1; ++k) {
                        st.act[k] = st.act[k + 1];
                        st.coef[k] = st.coef[k + 1];
                        st.ls[k] = st.ls[k + 1];
                        pos[st.act[k]] = k;
                    }
                    pos[fd] = na - 1;
                    cov[fd] = cov0[fd] - t;
                }
                --na;
                ++n_drop;
                wave_sync();
            }
            if (n_drop - drops_before > 1) ++n_multi;
        }
    }
    // the code: the last assignment, or its interpolation towards alpha_min
    if (a.code || a.proba) {
        double *out_code = a.code ? a.code + row * (int64_t)M : nullptr;
        if (interp) {
            // coef = prev + ss (coef - prev) over the union of both supports
            for (int j = lane; j < ncur; j += 64) {
                const int f = st.fa(cur)[j];
                double p = 0.0;
                for (int q = 0; q < nprev; ++q)
                    if (st.fa(cur ^ 1)[q] == f) p = st.va(cur ^ 1)[q];
                st.y[j] = p + ss * (st.va(cur)[j] - p);
            }
            wave_sync();
            for (int j = lane; j < ncur; j += 64) st.va(cur)[j] = st.y[j];
            int extra = 0;
            wave_sync();
            if (lane == 0) {
                for (int q = 0; q < nprev; ++q) {
                    const int f = st.fa(cur ^ 1)[q];
                    bool in = false;
                    for (int j = 0; j < ncur; ++j) in |= st.fa(cur)[j] == f;
                    if (!in) {
                        const double p = st.va(cur ^ 1)[q];
                        st.fa(cur)[ncur + extra] = f;
                        st.va(cur)[ncur + extra] = p + ss * (0.0 - p);
                        ++extra;
                    }
                }
            }
            wave_sync();
            extra = __shfl(extra, 0, 64);
            ncur += extra;
        }
        if (out_code) {
            for (int f = lane; f < M; f += 64) out_code[f] = 0.0;
            wave_sync();
            for (int j = lane; j < ncur; j += 64) out_code[st.fa(cur)[j]] = st.va(cur)[j];
        }
        if (a.proba) {
            const int C = a.C;
            double *pr = a.proba + row * (int64_t)C;
            double tot = 0.0;
            for (int c = lane; c < C; c += 64) {
                double r = 0.0;
                for (int j = 0; j < ncur; ++j) r += st.va(cur)[j] * a.P[(int64_t)st.fa(cur)[j] * C + c];
                tot += r;
            }
            tot = wave_sum(tot);
            for (int c = lane; c < C; c += 64) {
                double r = 0.0;
                for (int j = 0; j < ncur; ++j) r += st.va(cur)[j] * a.P[(int64_t)st.fa(cur)[j] * C + c];
                pr[c] = r / tot;
            }
        }
    }
    if (lane == 0) {
        atomicAdd(&a.counts[CNT_SAMPLES], 1ull);
        atomicAdd(&a.counts[CNT_ITERS], (unsigned long long)n_iter);
        atomicMax(&a.counts[CNT_ITER_MAX], (unsigned long long)n_iter);
        if (n_drop) atomicAdd(&a.counts[CNT_DROPS], n_drop);
        if (n_deg) atomicAdd(&a.counts[CNT_DEGENERATE], n_deg);
        if (n_early) atomicAdd(&a.counts[CNT_EARLY], n_early);
        if (n_retry) atomicAdd(&a.counts[CNT_AA_RETRY], n_retry);
        atomicMax(&a.counts[CNT_ACTIVE_MAX], (unsigned long long)max_act);
        if (n_multi) atomicAdd(&a.counts[CNT_MULTI_DROP], n_multi);
        atomicAdd(&a.counts[CNT_G_ROWS], g_rows);
    }
    return true;
}

__device__ inline void carve(ActiveSet &st, double *base, int cap) {
    double *p = base;
    st.L = p; p += lpk_size(cap);
    st.coef = p; p += cap + 1;
    st.ls = p; p += cap + 1;
    st.y = p; p += 2 * cap + 2;
    st.dg = p; p += cap + 1;
    st.va0 = p; p += 2 * cap + 2;
    st.va1 = p; p += 2 * cap + 2;
    int *q = reinterpret_cast<int *>(p);
    st.fa0 = q; q += 2 * cap + 2;
    st.fa1 = q; q += 2 * cap + 2;
    st.act = q;
}
__host__ __device__ constexpr int64_t slot_doubles(int64_t cap) {
    return lpk_size(cap) + 3 * (cap + 1) + 3 * (2 * cap + 2) + (5 * cap + 5 + 1) / 2;
}

__global__ __launch_bounds__(64) void sc_lars_kernel(LarsArgs a) {
    __shared__ __attribute__((aligned(16))) double lds[slot_doubles(SC_CAP)];
    ActiveSet st;
    carve(st, lds, SC_CAP);
    const int lane = threadIdx.x;
    for (int64_t row = blockIdx.x; row < a.rows; row += gridDim.x) {
        if (!lars_row(a, row, st, a.cap, lane)) {
            if (lane == 0) {
                const uint32_t t = atomicAdd(a.ovf_n, 1u);
                a.ovf_list[t] = (int32_t)row;
                atomicAdd(&a.counts[CNT_OVERFLOW], 1ull);
            }
        }
        wave_sync();
    }
}

// overflow passes: the listed rows again, the active set in a global slot of `slot_cap`; a row that outgrows
// it too is listed for the next pass (the last pass's cap, min(M, max_iter), always suffices)
__global__ __launch_bounds__(64) void sc_lars_overflow_kernel(LarsArgs a, const int32_t *in_list, const uint32_t *in_n,
                                                              int32_t *out_list, uint32_t *out_n, int slot_cap) {
    ActiveSet st;
    carve(st, a.slot_ws + (int64_t)blockIdx.x * slot_doubles(slot_cap), slot_cap);
    const int lane = threadIdx.x;
    const uint32_t n = *in_n;
    for (uint32_t t = blockIdx.x; t < n; t += gridDim.x) {
        if (!lars_row(a, in_list[t], st, slot_cap, lane) && lane == 0) {
            const uint32_t u = atomicAdd(out_n, 1u);
            out_list[u] = in_list[t];
        }
        wave_sync();
    }
}

// optional per-stage timing (bench / profiling): events around the stages of every call, accumulated
struct ScTimer {
    bool enabled = false, created = false;
    hipEvent_t ev[6];
    double ms[5] = {0, 0, 0, 0, 0};
};
ScTimer g_sc_timer;

struct ScWs {
    double *Wn, *G, *Xn, *cov0, *cov, *ced, *slots;
    int32_t *pos, *ovf_list, *ovf2_list;
    uint32_t *ovf_n;                    // [0]: rows of the first overflow pass, [1]: of the second
    int64_t slot_cap[2], n_slots[2];
};

// bytes of overflow slots per pass: the first pass takes every row past the LDS cap (several % of the rows on
// large maps), the second only the rare rows past SC_CAP1, whose slots are large (min(M, max_iter) entries)
constexpr int64_t SC_SLOT_BUDGET[2] = {(int64_t)256 << 20, (int64_t)32 << 20};
constexpr int64_t SC_CAP1 = 192;                         // active-set cap of the first overflow pass

size_t carve_ws(ScWs *w, char *base, int64_t Nq, int64_t d, int64_t M, int max_iter) {
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = base ? base + off : nullptr; off += align_up(bytes); return p; };
    w->slot_cap[1] = std::max<int64_t>(1, std::min<int64_t>(M, max_iter));
    w->slot_cap[0] = std::min(w->slot_cap[1], SC_CAP1);
    int64_t sb = 0;
    for (int p = 0; p < 2; ++p) {
        const int64_t b = slot_doubles(w->slot_cap[p]) * 8;
        w->n_slots[p] = std::max<int64_t>(1, std::min<int64_t>({(int64_t)4096, SC_SLOT_BUDGET[p] / b, std::max<int64_t>(Nq, 1)}));
        sb = std::max(sb, w->n_slots[p] * b);  // the passes run one after the other on one region
    }
    w->ovf_n = reinterpret_cast<uint32_t *>(take(256));
    w->Wn = reinterpret_cast<double *>(take((size_t)M * d * 8));
    w->G = reinterpret_cast<double *>(take((size_t)M * M * 8));
    w->Xn = reinterpret_cast<double *>(take((size_t)Nq * d * 8));
    w->cov0 = reinterpret_cast<double *>(take((size_t)Nq * M * 8));
    w->cov = reinterpret_cast<double *>(take((size_t)Nq * M * 8));
    w->ced = reinterpret_cast<double *>(take((size_t)Nq * M * 8));
    w->pos = reinterpret_cast<int32_t *>(take((size_t)Nq * M * 4));
    w->ovf_list = reinterpret_cast<int32_t *>(take((size_t)Nq * 4 + 4));
    w->ovf2_list = reinterpret_cast<int32_t *>(take((size_t)Nq * 4 + 4));
    w->slots = reinterpret_cast<double *>(take((size_t)sb));
    return off;
}

}  // namespace

}  // namespace dbgsom

using namespace dbgsom;

extern "C" {

size_t dbgsom_sparse_code_workspace_bytes(int64_t Nq, int64_t d, int64_t M, int max_iter) {
    if (Nq < 0 || d < 1 || M < 1 || max_iter < 0) return 0;
    ScWs w;
    return carve_ws(&w, nullptr, Nq, d, M, max_iter);
}

int dbgsom_sparse_code(const void *Xq, int x_dtype, int64_t Nq, int64_t d, int64_t ldx, const double *W, int64_t M,
                       int64_t ldw, int max_iter, int cap, const double *P, int64_t C, double *code, double *proba,
                       uint64_t *counts, void *ws, size_t ws_bytes, void *stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    DBGSOM_REQUIRE(x_dtype == DBGSOM_F32 || x_dtype == DBGSOM_F64, "x_dtype must be DBGSOM_F32 or DBGSOM_F64");
    DBGSOM_REQUIRE(Nq >= 0 && d >= 1 && M >= 1 && ldx >= d && ldw >= d, "bad shape");
    DBGSOM_REQUIRE(Nq <= 0x7fffffff && M <= 0x7fffffff && d <= 0x7fffffff, "shape too large");
    DBGSOM_REQUIRE(max_iter >= 0, "max_iter must be >= 0");
    DBGSOM_REQUIRE(cap >= 0, "cap must be >= 0 (0 = the library's fast-path cap)");
    DBGSOM_REQUIRE(W && counts && (Nq == 0 || Xq), "null pointer");
    DBGSOM_REQUIRE(!proba || (P && C >= 1 && C <= 0x7fffffff), "proba needs P and C >= 1");
    DBGSOM_REQUIRE(ws || ws_bytes == 0, "null workspace");
    DBGSOM_REQUIRE(ws_bytes >= dbgsom_sparse_code_workspace_bytes(Nq, d, M, max_iter), "workspace too small");
    DBGSOM_REQUIRE(is_aligned(ws, 256), "workspace must be 256-byte aligned");
    if (Nq == 0) return DBGSOM_OK;
    ScWs w;
    carve_ws(&w, static_cast<char *>(ws), Nq, d, M, max_iter);
    DBGSOM_HIP_CHECK(hipMemsetAsync(w.ovf_n, 0, 16, stream));
    ScTimer &tm = g_sc_timer;
    if (tm.enabled && !tm.created) {
        for (auto &e : tm.ev) DBGSOM_HIP_CHECK(hipEventCreate(&e));
        tm.created = true;
    }
    const bool timed = tm.enabled;
    auto stamp = [&](int i) { return timed ? hipEventRecord(tm.ev[i], stream) : hipSuccess; };
    DBGSOM_HIP_CHECK(stamp(0));
    hipLaunchKernelGGL(sc_normalize_kernel<double>, dim3((unsigned)M), dim3(64), 0, stream, W, M, (int)d, ldw, w.Wn, d);
    {
        int rc = launch_status("sc_normalize_kernel");
        if (rc) return rc;
        if ((rc = launch_gemm_nt(w.Wn, M, d, w.Wn, M, d, d, w.G, M, stream))) return rc;
    }
    DBGSOM_HIP_CHECK(stamp(1));
    if (x_dtype == DBGSOM_F32)
        hipLaunchKernelGGL(sc_normalize_kernel<float>, dim3((unsigned)Nq), dim3(64), 0, stream,
                           static_cast<const float *>(Xq), Nq, (int)d, ldx, w.Xn, d);
    else
        hipLaunchKernelGGL(sc_normalize_kernel<double>, dim3((unsigned)Nq), dim3(64), 0, stream,
                           static_cast<const double *>(Xq), Nq, (int)d, ldx, w.Xn, d);
    {
        int rc = launch_status("sc_normalize_kernel");
        if (rc) return rc;
        if ((rc = launch_gemm_nt(w.Xn, Nq, d, w.Wn, M, d, d, w.cov0, M, stream))) return rc;
    }
    DBGSOM_HIP_CHECK(stamp(2));
    LarsArgs a;
    a.G = w.G; a.cov0 = w.cov0; a.cov = w.cov; a.ced = w.ced; a.pos = w.pos;
    a.M = (int)M; a.d = (int)d; a.max_iter = max_iter;
    a.cap = cap == 0 ? SC_CAP : std::min(cap, SC_CAP);
    a.rows = Nq; a.P = P; a.C = (int)C; a.code = code; a.proba = proba;
    a.counts = reinterpret_cast<unsigned long long *>(counts);
    a.ovf_list = w.ovf_list; a.ovf_n = w.ovf_n;
    a.slot_ws = w.slots;
    const unsigned grid = (unsigned)std::min<int64_t>(Nq, (int64_t)1 << 20);
    hipLaunchKernelGGL(sc_lars_kernel, dim3(grid), dim3(64), 0, stream, a);
    if (const int rc = launch_status("sc_lars_kernel")) return rc;
    DBGSOM_HIP_CHECK(stamp(3));
    hipLaunchKernelGGL(sc_lars_overflow_kernel, dim3((unsigned)w.n_slots[0]), dim3(64), 0, stream, a, w.ovf_list,
                       w.ovf_n, w.ovf2_list, w.ovf_n + 1, (int)w.slot_cap[0]);
    if (const int rc = launch_status("sc_lars_overflow_kernel")) return rc;
    DBGSOM_HIP_CHECK(stamp(4));
    hipLaunchKernelGGL(sc_lars_overflow_kernel, dim3((unsigned)w.n_slots[1]), dim3(64), 0, stream, a, w.ovf2_list,
                       w.ovf_n + 1, w.ovf_list, w.ovf_n + 2, (int)w.slot_cap[1]);
    if (const int rc = launch_status("sc_lars_overflow_kernel")) return rc;
    if (timed) {  // (timing makes the call blocking)
        DBGSOM_HIP_CHECK(stamp(5));
        DBGSOM_HIP_CHECK(hipEventSynchronize(tm.ev[5]));
        for (int i = 0; i < 5; ++i) {
            float ms = 0.0f;
            DBGSOM_HIP_CHECK(hipEventElapsedTime(&ms, tm.ev[i], tm.ev[i + 1]));
            tm.ms[i] += ms;
        }
    }
    return DBGSOM_OK;
}

int dbgsom_sparse_code_timing(int enable) {
    g_sc_timer.enabled = enable != 0;
    for (double &m : g_sc_timer.ms) m = 0.0;
    return DBGSOM_OK;
}

int dbgsom_sparse_code_stage_ms(double *ms5) {
    DBGSOM_REQUIRE(ms5, "null pointer");
    for (int i = 0; i < 5; ++i) ms5[i] = g_sc_timer.ms[i];
    return DBGSOM_OK;
}

}  // extern "C"
