// The map read as an isotropic Gaussian mixture on gfx950 (MI355X): per row the log-sum-exp of t_j = a_j - c r_ij, the
// unit of the largest t_j and the posterior mean of up to 16 per-unit values, with a_j the log-priors, c = 1 / (2 h^2)
// and r_ij = max((|x_i|^2 + (-2 <x_i, w_j>)) + |w_j|^2, 0) the squared value of the search's own chain, without the
// N x M matrix ever leaving the chip's caches.
//
// Two kernels per slab of rows, on one stream, as distortion.hip:
//   1. the squared form of distances.hip: slab_rows x M values of r into the workspace, ordinary stores;
//   2. mixture_rows_kernel<V>: one wavefront per row finds (T, b), then sums s_j = exp(t_j - T) and s_j Y[j, v].
//
// The arithmetic is fixed so that NumPy restates it up to the library's exp and log:
//   t_j    a_j - (c * r_j): the product rounded, then the difference rounded (never a fused multiply-add);
//   (T, b) the largest t_j, lowest j among equals, over t_j > -inf and not NaN -- the smallest (-t_j, j) in
//          lexicographic order among -t_j < +inf; none: (b, lse, q) = (-1, NaN, NaN);
//   s_j    exp(t_j - T), the device library's float64 exp;
//   S, Q_v lane l's partials, from +0.0, over j = l, l + 64, ... ascending: S_l = S_l + s_j and Q_lv = Q_lv +
//          (s_j * Y[j, v]), the product rounded, then the sum rounded; then six rounds m = 1, 2, 4, 8, 16, 32 in which
//          every lane takes p_l + p_(l ^ m), as energy_rows_kernel;
//   lse    T + log(S);  q_v = Q_v / S, one division per row and value.
// Otherwise plain IEEE: a NaN t_j is never the maximum but enters the sums as it is.
//
// Lane l streams the entries l, l + 64, ... of its row (coalesced, four loads in flight).  The t of the first four stay
// in registers between the passes -- a map of up to 256 prototypes is read once -- and what lies beyond them is read
// again in pass 2 and its t formed again (the same two roundings: the same bits): the row was just written by the
// product kernel and sits in L2.  a (M values) and Y (M x V) are read through L2 by every wavefront; they are a few
// KiB and stay in cache.  Nothing of a row past M, and no column of Y past n_values, is read.
#include <math.h>

#include <algorithm>

#include "wave_lex.h"

namespace dbgsom {

constexpr int MIXTURE_NT = 256;            // four wavefronts, four rows per workgroup
constexpr int MIXTURE_EMPTY = TOPK_EMPTY;  // the index of a lane that saw no t above -inf

// a - (c * r): two roundings
__device__ __forceinline__ double mixture_t(double a, double c, double r) {
#pragma clang fp contract(off)
    const double p = __dmul_rn(c, r);
    return __dadd_rn(a, -p);
}

// p + (s * y): two roundings
__device__ __forceinline__ double mixture_term(double p, double s, double y) {
#pragma clang fp contract(off)
    const double t = __dmul_rn(s, y);
    return __dadd_rn(p, t);
}

// R: N rows of M squared values, ldr >= M apart.  a: M log-priors.  Y: M rows of nv <= V values, ldy >= nv apart.
// unit, lse: N values each.  q: N rows of nv values, ldq >= nv apart.
template <int V>
__global__ __launch_bounds__(MIXTURE_NT) void mixture_rows_kernel(const double *__restrict__ R, int64_t N, int M, int64_t ldr,
                                                                  const double *__restrict__ a, double c,
                                                                  const double *__restrict__ Y, int nv, int64_t ldy,
                                                                  int64_t *__restrict__ unit, double *__restrict__ lse,
                                                                  double *__restrict__ q, int64_t ldq) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (MIXTURE_NT / 64) + (threadIdx.x >> 6);
    if (row >= N) return;   // (wave-uniform: the wavefronts that stay are whole)
    const double *__restrict__ p = R + row * ldr;

    // pass 1: the lane's smallest (-t, j); the index ascends, so the strict '<' keeps the lowest among equal t.  A lane
    // without an entry at jj takes t = -inf, which never wins; neither does NaN.
    double bv = INFINITY;
    int bj = MIXTURE_EMPTY;
    double t0[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int jj = lane + 64 * u;
        t0[u] = (jj < M) ? mixture_t(a[jj], c, p[jj]) : -(double)INFINITY;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (-t0[u] < bv) { bv = -t0[u]; bj = lane + 64 * u; }
    for (int j0 = lane + 256; j0 < M + lane; j0 += 256) {   // (the trip count is wave-uniform; M + 63 + 256 < 2^31)
        double t[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int jj = j0 + 64 * u;
            t[u] = (jj < M) ? mixture_t(a[jj], c, p[jj]) : -(double)INFINITY;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (-t[u] < bv) { bv = -t[u]; bj = j0 + 64 * u; }
    }
    wave_lex_min(bv, bj);
    if (bj == MIXTURE_EMPTY) {   // (wave-uniform) no unit with mass
        if (lane == 0) {
            unit[row] = -1;
            lse[row] = NAN;
            for (int v = 0; v < nv; ++v) q[row * ldq + v] = NAN;
        }
        return;
    }
    const double T = -bv;

    // pass 2: the lane's partials over its entries, ascending; a lane without an entry at jj adds nothing
    double S = 0.0;
    double Q[V > 0 ? V : 1];
#pragma unroll
    for (int v = 0; v < V; ++v) Q[v] = 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int jj = lane + 64 * u;
        if (jj < M) {
            const double s = exp(t0[u] - T);
            S = __dadd_rn(S, s);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const double y = (v < nv) ? Y[(int64_t)jj * ldy + v] : 0.0;
                Q[v] = mixture_term(Q[v], s, y);
            }
        }
    }
    for (int j0 = lane + 256; j0 < M + lane; j0 += 256) {
        double t[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int jj = j0 + 64 * u;
            t[u] = (jj < M) ? mixture_t(a[jj], c, p[jj]) : -(double)INFINITY;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int jj = j0 + 64 * u;
            if (jj < M) {
                const double s = exp(t[u] - T);
                S = __dadd_rn(S, s);
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const double y = (v < nv) ? Y[(int64_t)jj * ldy + v] : 0.0;
                    Q[v] = mixture_term(Q[v], s, y);
                }
            }
        }
    }
    // the butterfly: both lanes of a pair form the same sum, so after six rounds every lane holds S and every Q_v
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        S = __dadd_rn(S, __shfl_xor(S, m));
#pragma unroll
        for (int v = 0; v < V; ++v) Q[v] = __dadd_rn(Q[v], __shfl_xor(Q[v], m));
    }
    if (lane == 0) {
        unit[row] = bj;
        lse[row] = T + log(S);
#pragma unroll
        for (int v = 0; v < V; ++v)
            if (v < nv) q[row * ldq + v] = Q[v] / S;
    }
}

// ---------------------------------------------------------------------------------------------
static int mixture_check(int64_t N, int64_t M, int64_t ldr, double c, int n_values, int64_t ldy, int64_t ldq) {
    DBGSOM_REQUIRE(N >= 0, "bad sample shape");
    DBGSOM_REQUIRE(M >= 1 && M <= DBGSOM_MAX_PROTOTYPES, "need 1 <= M <= DBGSOM_MAX_PROTOTYPES");
    DBGSOM_REQUIRE(ldr >= M, "ldr must be >= M");
    DBGSOM_REQUIRE(n_values >= 0 && n_values <= DBGSOM_MAX_MIXTURE_VALUES, "need 0 <= n_values <= DBGSOM_MAX_MIXTURE_VALUES");
    DBGSOM_REQUIRE(ldy >= n_values, "ldy must be >= n_values");
    DBGSOM_REQUIRE(ldq >= n_values, "ldq must be >= n_values");
    DBGSOM_REQUIRE(c >= 0.0, "c must be >= 0");   // (NaN fails)
    return DBGSOM_OK;
}

static int mixture_check_pointers(const double *a, const double *Y, int n_values, const int64_t *unit, const double *lse,
                                  const double *q) {
    DBGSOM_REQUIRE(a && unit && lse && (n_values == 0 || (Y && q)), "null pointer");
    DBGSOM_REQUIRE(is_aligned(a, 8) && is_aligned(Y, 8) && is_aligned(unit, 8) && is_aligned(lse, 8) && is_aligned(q, 8),
                   "pointers must be 8-byte aligned");
    return DBGSOM_OK;
}

template <int V>
static void mixture_rows_launch(unsigned nb, hipStream_t s, const double *R, int64_t N, int M, int64_t ldr, const double *a,
                                double c, const double *Y, int nv, int64_t ldy, int64_t *unit, double *lse, double *q,
                                int64_t ldq) {
    hipLaunchKernelGGL(mixture_rows_kernel<V>, dim3(nb), dim3(MIXTURE_NT), 0, s, R, N, M, ldr, a, c, Y, nv, ldy, unit, lse, q,
                       ldq);
}

int launch_mixture_rows(const double *R, int64_t N, int64_t M, int64_t ldr, const double *a, double c, const double *Y,
                        int n_values, int64_t ldy, int64_t *unit, double *lse, double *q, int64_t ldq, hipStream_t s) {
    TRY_STATUS(mixture_check(N, M, ldr, c, n_values, ldy, ldq));
    if (N == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(R, "null pointer");
    TRY_STATUS(mixture_check_pointers(a, Y, n_values, unit, lse, q));
    DBGSOM_REQUIRE(is_aligned(R, 8), "pointers must be 8-byte aligned");
    const int64_t nb64 = (N + MIXTURE_NT / 64 - 1) / (MIXTURE_NT / 64);
    DBGSOM_REQUIRE(nb64 <= 0x7fffffff, "too many samples for one launch");
    const unsigned nb = (unsigned)nb64;
    const int m = (int)M;
    // the smallest instance that holds n_values; its surplus columns are guarded in the kernel
    if (n_values == 0) mixture_rows_launch<0>(nb, s, R, N, m, ldr, a, c, Y, n_values, ldy, unit, lse, q, ldq);
    else if (n_values == 1) mixture_rows_launch<1>(nb, s, R, N, m, ldr, a, c, Y, n_values, ldy, unit, lse, q, ldq);
    else if (n_values == 2) mixture_rows_launch<2>(nb, s, R, N, m, ldr, a, c, Y, n_values, ldy, unit, lse, q, ldq);
    else if (n_values <= 4) mixture_rows_launch<4>(nb, s, R, N, m, ldr, a, c, Y, n_values, ldy, unit, lse, q, ldq);
    else if (n_values <= 8) mixture_rows_launch<8>(nb, s, R, N, m, ldr, a, c, Y, n_values, ldy, unit, lse, q, ldq);
    else mixture_rows_launch<16>(nb, s, R, N, m, ldr, a, c, Y, n_values, ldy, unit, lse, q, ldq);
    return launch_status("mixture_rows_kernel");
}

// the Euclidean slab loop (the slab size rule and the workspace of launch_kneighbors) with the mixture kernel behind the
// product
int launch_mixture(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx, const double *W, int64_t M,
                   const double *ww, const double *a, double c, const double *Y, int n_values, int64_t ldy, int64_t slab_rows,
                   int64_t *unit, double *lse, double *q, int64_t ldq, void *ws, size_t ws_bytes, hipStream_t s) {
    DBGSOM_REQUIRE(valid_dtype(x_dtype), "x_dtype must be DBGSOM_F32/F64/BF16");
    DBGSOM_REQUIRE(N >= 0 && d >= 1 && ldx >= d && d <= 0x7fffffff, "bad sample shape");
    TRY_STATUS(mixture_check(N, M, M, c, n_values, ldy, ldq));
    DBGSOM_REQUIRE(slab_rows >= 0, "slab_rows must be >= 0 (0 = the default)");
    if (N == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(X && xx && W && ww && ws, "null pointer");
    TRY_STATUS(mixture_check_pointers(a, Y, n_values, unit, lse, q));
    TRY_STATUS(kneighbors_workspace_check("dbgsom_mixture", N, M, slab_rows, ws, ws_bytes, 0));
    return euclidean_slabs(X, x_dtype, N, d, ldx, xx, W, M, ww, slab_rows, static_cast<double *>(ws), s,
                           [&](int64_t r0, int64_t n, const double *slab, int64_t ldr) {
                               return launch_mixture_rows(slab, n, M, ldr, a, c, Y, n_values, ldy, unit + r0, lse + r0,
                                                          q ? q + r0 * ldq : nullptr, ldq, s);
                           });
}

}  // namespace dbgsom

using namespace dbgsom;

extern "C" {

int dbgsom_mixture_rows(const double *R_dev, int64_t N, int64_t M, int64_t ldr, const double *logprior_dev, double c,
                        const double *Y_dev, int n_values, int64_t ldy, int64_t *unit_dev, double *lse_dev, double *q_dev,
                        int64_t ldq, void *stream) {
    return launch_mixture_rows(R_dev, N, M, ldr, logprior_dev, c, Y_dev, n_values, ldy, unit_dev, lse_dev, q_dev, ldq,
                               (hipStream_t)stream);
}

int dbgsom_mixture(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx_dev,
                   const double *W_dev, int64_t M, const double *ww_dev, const double *logprior_dev, double c,
                   const double *Y_dev, int n_values, int64_t ldy, int64_t slab_rows, int64_t *unit_dev, double *lse_dev,
                   double *q_dev, int64_t ldq, void *workspace_dev, size_t workspace_bytes, void *stream) {
    return launch_mixture(X_dev, x_dtype, N, d, ldx, xx_dev, W_dev, M, ww_dev, logprior_dev, c, Y_dev, n_values, ldy,
                          slab_rows, unit_dev, lse_dev, q_dev, ldq, workspace_dev, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
