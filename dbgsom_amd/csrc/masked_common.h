// Pieces shared by the masked search (masked.hip) and its sibling that stores every distance (distances.hip).
#pragma once
#include "common.h"

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

// ---- search ---------------------------------------------------------------------------------------------
// U features of R rows against this lane's prototype: acc[r] goes on along its chain, k ascending.  The skip of a
// missing entry has to stay a branch of the scalar unit: as a select it would cost two more vector instructions
// per entry than the arithmetic itself (the empty asm keeps the compiler from turning it into one).
template <int R, int U>
__device__ __forceinline__ void masked_step(const double *__restrict__ xb, const uint32_t (&off)[R], int e,
                                            const double *__restrict__ wcol, int64_t ldwt, double (&acc)[R]) {
    double w[U];
#pragma unroll
    for (int u = 0; u < U; ++u) w[u] = wcol[(int64_t)(e + u) * ldwt];
    // (uniform: the same entries for every lane; the next row's load is in flight while this row is worked on)
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
        for (int u = 0; u < U; ++u) {
            if (!nan_bits_uniform(x[u])) {
                double t = x[u] - w[u];
                asm volatile("" : "+v"(t));
                acc[r] = fma(t, t, acc[r]);
            }
        }
    }
}

}  // namespace dbgsom
