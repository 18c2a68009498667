// Pieces shared by the two BMU kernels (bmu.hip: register-staged, any shape; bmu_dma.hip:
// LDS-DMA ring for 16-byte aligned rows with d % 16 == 0) and by their siblings that store every
// distance (distances.hip).
#pragma once
#include <math.h>

#include "common.h"

namespace dbgsom {

typedef double d4_t __attribute__((ext_vector_type(4)));

constexpr int BI = 128;     // samples per workgroup
constexpr int BJ = 128;     // prototypes per sweep chunk
constexpr int KT = 16;      // feature depth of one LDS tile
constexpr int NT = 256;

// What the chunk epilogue of the four MFMA kernels makes of a pair's dot product a = <x_i, w_j>.  L2: the clamped
// squared distance (|x|^2 + (-2 a)) + |w|^2.  COSINE: the kernels receive u_i = inv(|x_i|^2) where they take xx and
// v_j = inv(|w_j|^2) where they take ww (cosine.hip: inv_norms_kernel), and the value is pair_value_cosine.
enum class Metric { L2, COSINE };

// c = 1 - (a u) v clamped to [0, 2], NaN kept: three roundings, never a fused multiply-add (the library is built
// with -ffp-contract=on, which would make one of 1 - t v)
__device__ __forceinline__ double pair_value_cosine(double a, double u, double v) {
#pragma clang fp contract(off)
    const double t = a * u;
    const double s = t * v;
    double c = 1.0 - s;
    if (c > 2.0) c = 2.0;
    if (!(c > 0.0)) c = (c != c) ? c : 0.0;
    return c;
}

__device__ __forceinline__ bool lex_lt(double a, int ja, double b, int jb) {
    return a < b || (a == b && ja < jb);
}

template <int K>
struct Best {
    double v[K];
    int j[K];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int t = 0; t < K; ++t) { v[t] = INFINITY; j[t] = 0x7fffffff; }
    }
    // candidates arrive with ascending index inside one lane: strict '<' keeps the lowest index
    __device__ __forceinline__ void push(double r, int idx) {
        if constexpr (K == 1) {
            if (r < v[0]) { v[0] = r; j[0] = idx; }
        } else {
            if (r < v[0]) { v[1] = v[0]; j[1] = j[0]; v[0] = r; j[0] = idx; }
            else if (r < v[1]) { v[1] = r; j[1] = idx; }
        }
    }
    // merge with another sorted list (lexicographic on (value, index))
    __device__ __forceinline__ void merge(const double (&ov)[K], const int (&oj)[K]) {
        if constexpr (K == 1) {
            if (lex_lt(ov[0], oj[0], v[0], j[0])) { v[0] = ov[0]; j[0] = oj[0]; }
        } else {
            double n0, n1; int m0, m1;
            if (lex_lt(ov[0], oj[0], v[0], j[0])) {
                n0 = ov[0]; m0 = oj[0];
                if (lex_lt(v[0], j[0], ov[1], oj[1])) { n1 = v[0]; m1 = j[0]; }
                else { n1 = ov[1]; m1 = oj[1]; }
            } else {
                n0 = v[0]; m0 = j[0];
                if (lex_lt(ov[0], oj[0], v[1], j[1])) { n1 = ov[0]; m1 = oj[0]; }
                else { n1 = v[1]; m1 = j[1]; }
            }
            v[0] = n0; j[0] = m0; v[1] = n1; j[1] = m1;
        }
    }
};


int launch_bmu_dma(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx,
                   const double *W, int64_t M, const double *ww, int k, int round_f32,
                   int64_t *idx, double *dist, hipStream_t s);
int launch_bmu_dma_cosine(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *u,
                          const double *W, int64_t M, const double *v, int k, int64_t *idx, double *dist,
                          hipStream_t s);
bool bmu_dma_usable(const void *X, int x_dtype, int64_t d, int64_t ldx, const void *W, int64_t M);
// 16-prototype tiles per wavefront of the LDS-DMA form for a map of M prototypes (1, 2 or 4; 0: register-staged)
int dma_chunk_tiles(int x_dtype, int64_t M);

}  // namespace dbgsom
