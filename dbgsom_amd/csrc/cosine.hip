// metric="cosine" on gfx950 (MI355X): what belongs to the metric alone.
//
// The cosine distance of row x_i to prototype w_j is
//     c_ij = 1 - (a_ij u_i) v_j,  clamped to [0, 2] (NaN stays NaN),
// with a_ij = <x_i, w_j> the sequential fma chain of the Euclidean search (bmu.hip, oracle/bmu_chain.c) and
//     u_i = inv(|x_i|^2), v_j = inv(|w_j|^2),  inv(t) = 0 if t == 0; 1 / sqrt(t) if 0 < t < +inf; NaN otherwise,
// each operation rounded on its own in float64.  The product is the heavy part and is not here: the MFMA kernels of
// bmu.hip, bmu_dma.hip and distances.hip have a cosine form (template switch Metric::COSINE, bmu_common.h) that takes u
// where they take |x|^2 and v where they take |w|^2 and replaces the chunk epilogue.  Here: the kernel for inv() over
// a vector of squared norms -- N or M values, once per call, so that no epilogue pays a divide and a root per lane and
// chunk -- and the device-level C ABI of the metric.
//
// inv(0) = 0 makes a zero row (or one whose squared norm underflows to 0) a row at distance 1 from everything, the
// value scikit-learn gives; inv(+inf) = inv(NaN) = NaN makes a row with NaN or an infinity, or one whose squared norm
// overflows, a row of NaN that the search never reports (Best<K>::push takes values below +inf only).
#include <math.h>

#include "common.h"

namespace dbgsom {

// sqrt, then the division: two roundings (both correctly rounded in float64 here; no reciprocal square root)
__global__ __launch_bounds__(256) void inv_norms_kernel(const double *__restrict__ sq, int64_t n, double *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double t = sq[i];
        double r = NAN;
        if (t == 0.0) r = 0.0;
        else if (t > 0.0 && t < (double)INFINITY) r = 1.0 / sqrt(t);
        out[i] = r;
    }
}

int launch_inv_norms(const double *sq, int64_t n, double *out, hipStream_t s) {
    DBGSOM_REQUIRE(n >= 0, "bad n");
    if (n == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(sq && out, "null pointer");
    DBGSOM_REQUIRE(is_aligned(sq, 8) && is_aligned(out, 8), "pointers must be 8-byte aligned");
    const int64_t nb = (n + 255) / 256;
    hipLaunchKernelGGL(inv_norms_kernel, dim3((unsigned)(nb > 4096 ? 4096 : nb)), dim3(256), 0, s, sq, n, out);
    return launch_status("inv_norms_kernel");
}

}  // namespace dbgsom

using namespace dbgsom;

extern "C" {

int dbgsom_inv_norms(const double *sq_dev, int64_t n, double *out_dev, void *stream) {
    return launch_inv_norms(sq_dev, n, out_dev, (hipStream_t)stream);
}

int dbgsom_bmu_cosine(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *u_dev,
                      const double *W_dev, int64_t M, const double *v_dev, int k, int64_t *idx_dev, double *dist_dev,
                      void *stream) {
    return launch_bmu_cosine(X_dev, x_dtype, N, d, ldx, u_dev, W_dev, M, v_dev, k, idx_dev, dist_dev, (hipStream_t)stream);
}

int dbgsom_distances_cosine(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *u_dev,
                            const double *W_dev, int64_t M, const double *v_dev, double *out_dev, int64_t ldo,
                            void *stream) {
    return launch_distances_cosine(X_dev, x_dtype, N, d, ldx, u_dev, W_dev, M, v_dev, out_dev, ldo, (hipStream_t)stream);
}

size_t dbgsom_kneighbors_cosine_workspace_bytes(int64_t N, int64_t M, int64_t slab_rows) {
    return kneighbors_workspace_bytes(N, M, slab_rows);
}

int dbgsom_kneighbors_cosine(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *u_dev,
                             const double *W_dev, int64_t M, const double *v_dev, int k, int64_t slab_rows,
                             int64_t *idx_dev, double *dist_dev, void *workspace_dev, size_t workspace_bytes,
                             void *stream) {
    return launch_kneighbors_cosine(X_dev, x_dtype, N, d, ldx, u_dev, W_dev, M, v_dev, k, slab_rows, idx_dev, dist_dev,
                                    workspace_dev, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
