// Operand staging shared by the BMU kernels and their siblings that store every distance (distances.hip):
// the register-staged loads of bmu.hip and the LDS-DMA tiles of bmu_dma.hip.
#pragma once
#include "bmu_common.h"

namespace dbgsom {

// ---- register-staged form (bmu.hip, distances.hip) ----
constexpr int LS = KT + 2;  // LDS row stride (doubles)

template <typename T>
__device__ __forceinline__ void load8(const T *__restrict__ base, int64_t row, int64_t nrows,
                                      int64_t ld, int k, int d, int vec_ok, T (&v)[8]) {
    if (row < nrows && k < d) {
        const T *p = base + row * ld + k;
        if (vec_ok && k + 8 <= d) {
            if constexpr (sizeof(T) == 2) {
                const uint4 a = *reinterpret_cast<const uint4 *>(p);
                const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[2 * e].bits = (uint16_t)(w[e] & 0xffffu);
                    v[2 * e + 1].bits = (uint16_t)(w[e] >> 16);
                }
            } else if constexpr (sizeof(T) == 4) {
                const float4 a = *reinterpret_cast<const float4 *>(p);
                const float4 b = *reinterpret_cast<const float4 *>(p + 4);
                v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
                v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const double2 a = *reinterpret_cast<const double2 *>(p + 2 * e);
                    v[2 * e] = a.x;
                    v[2 * e + 1] = a.y;
                }
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (k + e < d) ? p[e] : T(0);
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = T(0);
    }
}

// ---- LDS-DMA form (bmu_dma.hip, distances.hip) ----
constexpr int NSTAGE = 3;

typedef __attribute__((address_space(3))) void *lds_ptr_t;
typedef const __attribute__((address_space(1))) void *gbl_ptr_t;

__device__ __forceinline__ void dma16(const void *src, void *lds_dst) {
    __builtin_amdgcn_global_load_lds((gbl_ptr_t)src, (lds_ptr_t)lds_dst, 16, 0, 0);
}

template <typename XT>
struct XTile {
    static constexpr int ROW_BYTES = KT * (int)sizeof(XT);  // 64 (f32) or 128 (f64)
    static constexpr int CHUNKS = ROW_BYTES / 16;            // 4 or 8
    static constexpr int BYTES = BI * ROW_BYTES;             // 8 KB or 16 KB
    static constexpr int DMA_PER_WAVE = BYTES / 1024 / 4;    // wave-instructions per tile per wave
};

constexpr int W_ROW_BYTES = KT * 8, W_CHUNKS = 8;

}  // namespace dbgsom
