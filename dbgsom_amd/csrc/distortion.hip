// The SOM distortion measure of every row on gfx950 (MI355X): e_i = sum_j h(b_i, j) r_ij with b_i the best matching
// unit of row i and r_ij = max((|x_i|^2 + (-2 <x_i, w_j>)) + |w_j|^2, 0) the squared value of the search's own chain,
// without the N x M matrix ever leaving the chip's caches.
//
// Two kernels per slab of rows, on one stream, as kneighbors.hip:
//   1. the squared form of distances.hip: slab_rows x M values of r into the workspace, ordinary stores;
//   2. energy_rows_kernel: one wavefront per row finds b, then sums row b of H against the row of r.
//
// The arithmetic is fixed so that NumPy restates it bit for bit:
//   b    the index of the smallest (r_j, j) in lexicographic order among r_j < +inf; none: (b, e) = (-1, NaN);
//   p_l  lane l's partial, from +0.0, over j = l, l + 64, ... ascending: p_l = p_l + (H[b, j] * r_j), the product
//        rounded, then the sum rounded (never a fused multiply-add);
//   e    six rounds m = 1, 2, 4, 8, 16, 32 in which every lane takes p_l + p_(l ^ m); then p_0.
// Otherwise plain IEEE: a +inf or NaN r_j enters the sum as it is (0 * inf = NaN).
//
// Lane l streams the entries l, l + 64, ... of its row (coalesced, four loads in flight).  The first four stay in
// registers between the passes -- a map of up to 256 prototypes is read once -- and what lies beyond them is read
// again in pass 2: it was just written by the product kernel and sits in L2.  Row b of H is read the same way; rows
// with the same unit share it in cache.  Nothing of a row past M is read.
#include <math.h>

#include <algorithm>

#include "wave_lex.h"

namespace dbgsom {

constexpr int ENERGY_NT = 256;            // four wavefronts, four rows per workgroup
constexpr int ENERGY_EMPTY = 0x7fffffff;  // the index of a lane that saw nothing below +inf (Best<K>::init)

// p + (h * r): two roundings
__device__ __forceinline__ double energy_term(double p, double h, double r) {
#pragma clang fp contract(off)
    const double t = __dmul_rn(h, r);
    return __dadd_rn(p, t);
}

// R: N rows of M squared values, ldr >= M apart.  H: M rows of M factors, ldh >= M apart.  bmu, e: N values each.
__global__ __launch_bounds__(ENERGY_NT) void energy_rows_kernel(const double *__restrict__ R, int64_t N, int M, int64_t ldr,
                                                                const double *__restrict__ H, int64_t ldh,
                                                                int64_t *__restrict__ bmu, double *__restrict__ e) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (ENERGY_NT / 64) + (threadIdx.x >> 6);
    if (row >= N) return;   // (wave-uniform: the wavefronts that stay are whole)
    const double *__restrict__ p = R + row * ldr;

    // pass 1: the lane's smallest (r, j); the index ascends, so the strict '<' keeps the lowest among equal r
    double bv = INFINITY;
    int bj = ENERGY_EMPTY;
    double r0[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int jj = lane + 64 * u;
        r0[u] = (jj < M) ? p[jj] : (double)INFINITY;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (r0[u] < bv) { bv = r0[u]; bj = lane + 64 * u; }
    for (int j0 = lane + 256; j0 < M + lane; j0 += 256) {   // (the trip count is wave-uniform; M + 63 + 256 < 2^31)
        double r[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int jj = j0 + 64 * u;
            r[u] = (jj < M) ? p[jj] : (double)INFINITY;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (r[u] < bv) { bv = r[u]; bj = j0 + 64 * u; }
    }
    wave_lex_min(bv, bj);
    if (bj == ENERGY_EMPTY) {   // (wave-uniform) nothing below +inf
        if (lane == 0) { bmu[row] = -1; e[row] = NAN; }
        return;
    }

    // pass 2: the lane's partial over its entries, ascending; a lane without an entry at jj adds nothing
    const double *__restrict__ h = H + (int64_t)bj * ldh;
    double acc = 0.0;
    {
        double h0[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int jj = lane + 64 * u;
            h0[u] = (jj < M) ? h[jj] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (lane + 64 * u < M) acc = energy_term(acc, h0[u], r0[u]);
    }
    for (int j0 = lane + 256; j0 < M + lane; j0 += 256) {
        double r[4], hh[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int jj = j0 + 64 * u;
            r[u] = (jj < M) ? p[jj] : 0.0;
            hh[u] = (jj < M) ? h[jj] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (j0 + 64 * u < M) acc = energy_term(acc, hh[u], r[u]);
    }
    // the butterfly: both lanes of a pair form the same sum, so after six rounds every lane holds e
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) acc = __dadd_rn(acc, __shfl_xor(acc, m));
    if (lane == 0) { bmu[row] = bj; e[row] = acc; }
}

// ---------------------------------------------------------------------------------------------
static int energy_check(int64_t N, int64_t M, int64_t ldr, int64_t ldh) {
    DBGSOM_REQUIRE(N >= 0, "bad sample shape");
    DBGSOM_REQUIRE(M >= 1 && M <= DBGSOM_MAX_PROTOTYPES, "need 1 <= M <= DBGSOM_MAX_PROTOTYPES");
    DBGSOM_REQUIRE(ldr >= M, "ldr must be >= M");
    DBGSOM_REQUIRE(ldh >= M, "ldh must be >= M");
    return DBGSOM_OK;
}

int launch_energy_rows(const double *R, int64_t N, int64_t M, int64_t ldr, const double *H, int64_t ldh, int64_t *bmu,
                       double *e, hipStream_t s) {
    TRY_STATUS(energy_check(N, M, ldr, ldh));
    if (N == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(R && H && bmu && e, "null pointer");
    DBGSOM_REQUIRE(is_aligned(R, 8) && is_aligned(H, 8) && is_aligned(bmu, 8) && is_aligned(e, 8),
                   "pointers must be 8-byte aligned");
    const int64_t nb = (N + ENERGY_NT / 64 - 1) / (ENERGY_NT / 64);
    DBGSOM_REQUIRE(nb <= 0x7fffffff, "too many samples for one launch");
    hipLaunchKernelGGL(energy_rows_kernel, dim3((unsigned)nb), dim3(ENERGY_NT), 0, s, R, N, (int)M, ldr, H, ldh, bmu, e);
    return launch_status("energy_rows_kernel");
}

// the Euclidean slab loop (the slab size rule and the workspace of launch_kneighbors) with the energy kernel behind the product
int launch_neighborhood_energy(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx,
                               const double *W, int64_t M, const double *ww, const double *H, int64_t ldh,
                               int64_t slab_rows, int64_t *bmu, double *e, void *ws, size_t ws_bytes, hipStream_t s) {
    DBGSOM_REQUIRE(valid_dtype(x_dtype), "x_dtype must be DBGSOM_F32/F64/BF16");
    DBGSOM_REQUIRE(N >= 0 && d >= 1 && ldx >= d && d <= 0x7fffffff, "bad sample shape");
    TRY_STATUS(energy_check(N, M, M, ldh));
    DBGSOM_REQUIRE(slab_rows >= 0, "slab_rows must be >= 0 (0 = the default)");
    if (N == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(X && xx && W && ww && H && bmu && e && ws, "null pointer");
    DBGSOM_REQUIRE(is_aligned(H, 8) && is_aligned(bmu, 8) && is_aligned(e, 8), "pointers must be 8-byte aligned");
    TRY_STATUS(kneighbors_workspace_check("dbgsom_neighborhood_energy", N, M, slab_rows, ws, ws_bytes, 0));
    return euclidean_slabs(X, x_dtype, N, d, ldx, xx, W, M, ww, slab_rows, static_cast<double *>(ws), s,
                           [&](int64_t r0, int64_t n, const double *slab, int64_t ldr) {
                               return launch_energy_rows(slab, n, M, ldr, H, ldh, bmu + r0, e + r0, s);
                           });
}

}  // namespace dbgsom

using namespace dbgsom;

extern "C" {

int dbgsom_energy_rows(const double *R_dev, int64_t N, int64_t M, int64_t ldr, const double *H_dev, int64_t ldh,
                       int64_t *bmu_dev, double *e_dev, void *stream) {
    return launch_energy_rows(R_dev, N, M, ldr, H_dev, ldh, bmu_dev, e_dev, (hipStream_t)stream);
}

int dbgsom_neighborhood_energy(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx_dev,
                               const double *W_dev, int64_t M, const double *ww_dev, const double *H_dev, int64_t ldh,
                               int64_t slab_rows, int64_t *bmu_dev, double *e_dev, void *workspace_dev,
                               size_t workspace_bytes, void *stream) {
    return launch_neighborhood_energy(X_dev, x_dtype, N, d, ldx, xx_dev, W_dev, M, ww_dev, H_dev, ldh, slab_rows, bmu_dev,
                                      e_dev, workspace_dev, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
