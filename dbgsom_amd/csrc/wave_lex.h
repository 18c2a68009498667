// The wave-wide lexicographic arg-min over (value, index) pairs, one pair per lane, without LDS, and the sorted list of
// K pairs a lane keeps in registers: shared by the selection kernels of kneighbors.hip and exemplars.hip and the energy
// kernel of distortion.hip.
#pragma once
#include "bmu_common.h"

namespace dbgsom {

constexpr int TOPK_EMPTY = 0x7fffffff;    // the index of an unfilled slot (Best<K>::init)

template <int K>
struct SortedList {
    double v[K];
    int j[K];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int t = 0; t < K; ++t) { v[t] = INFINITY; j[t] = TOPK_EMPTY; }
    }
    // (r, idx) takes its place behind every entry <= r; the last entry drops out.  NaN and +inf never enter.
    __device__ __forceinline__ void push(double r, int idx) {
        if (r < v[K - 1]) {
#pragma unroll
            for (int t = K - 1; t >= 1; --t) {
                const bool up = r < v[t - 1], here = r < v[t];
                v[t] = up ? v[t - 1] : (here ? r : v[t]);
                j[t] = up ? j[t - 1] : (here ? idx : j[t]);
            }
            if (r < v[0]) { v[0] = r; j[0] = idx; }
        }
    }
    // the same for pairs that arrive in any order of idx: (r, idx) takes its place by the lexicographic order
    __device__ __forceinline__ void push_lex(double r, int idx) {
        if (r < (double)INFINITY && lex_lt(r, idx, v[K - 1], j[K - 1])) {
#pragma unroll
            for (int t = K - 1; t >= 1; --t) {
                const bool up = lex_lt(r, idx, v[t - 1], j[t - 1]), here = lex_lt(r, idx, v[t], j[t]);
                v[t] = up ? v[t - 1] : (here ? r : v[t]);
                j[t] = up ? j[t - 1] : (here ? idx : j[t]);
            }
            if (lex_lt(r, idx, v[0], j[0])) { v[0] = r; j[0] = idx; }
        }
    }
    __device__ __forceinline__ void pop(bool won) {
#pragma unroll
        for (int t = 0; t + 1 < K; ++t) {
            v[t] = won ? v[t + 1] : v[t];
            j[t] = won ? j[t + 1] : j[t];
        }
        v[K - 1] = won ? (double)INFINITY : v[K - 1];
        j[K - 1] = won ? TOPK_EMPTY : j[K - 1];
    }
};

struct Head {
    uint32_t lo, hi;
    int j;
    __device__ __forceinline__ double value() const { return __hiloint2double((int)hi, (int)lo); }
};

__device__ __forceinline__ Head lex_min(const Head &a, const Head &b) {
    return lex_lt(b.value(), b.j, a.value(), a.j) ? b : a;
}

// the head of another lane of this row of 16 lanes (every lane is active: `old` is never taken)
template <int CTRL>
__device__ __forceinline__ Head from_lane(const Head &h) {
    Head o;
    o.lo = (uint32_t)__builtin_amdgcn_update_dpp((int)h.lo, (int)h.lo, CTRL, 0xf, 0xf, false);
    o.hi = (uint32_t)__builtin_amdgcn_update_dpp((int)h.hi, (int)h.hi, CTRL, 0xf, 0xf, false);
    o.j = __builtin_amdgcn_update_dpp(h.j, h.j, CTRL, 0xf, 0xf, false);
    return o;
}

// the lexicographic minimum of (v, j) over the 64 lanes, in every lane.  Each step folds in the lane (or the group
// already folded) across: lanes ^ 1, ^ 2 (quad_perm), the other quad of eight (row_half_mirror), the other half of
// sixteen (row_mirror), the neighbouring row of 16 (v_permlane16_swap: a's odd rows <-> b's even rows, so of (a, b)
// one is this lane's own and one the other row's), the other half of the wavefront (v_permlane32_swap likewise).
__device__ __forceinline__ void wave_lex_min(double &v, int &j) {
    constexpr int QUAD_1032 = 0xB1, QUAD_2301 = 0x4E, ROW_MIRROR = 0x140, ROW_HALF_MIRROR = 0x141;
    Head h{(uint32_t)__double2loint(v), (uint32_t)__double2hiint(v), j};
    h = lex_min(h, from_lane<QUAD_1032>(h));
    h = lex_min(h, from_lane<QUAD_2301>(h));
    h = lex_min(h, from_lane<ROW_HALF_MIRROR>(h));
    h = lex_min(h, from_lane<ROW_MIRROR>(h));
    {
        const auto lo = __builtin_amdgcn_permlane16_swap(h.lo, h.lo, false, false);
        const auto hi = __builtin_amdgcn_permlane16_swap(h.hi, h.hi, false, false);
        const auto jj = __builtin_amdgcn_permlane16_swap((uint32_t)h.j, (uint32_t)h.j, false, false);
        h = lex_min(Head{lo[0], hi[0], (int)jj[0]}, Head{lo[1], hi[1], (int)jj[1]});
    }
    {
        const auto lo = __builtin_amdgcn_permlane32_swap(h.lo, h.lo, false, false);
        const auto hi = __builtin_amdgcn_permlane32_swap(h.hi, h.hi, false, false);
        const auto jj = __builtin_amdgcn_permlane32_swap((uint32_t)h.j, (uint32_t)h.j, false, false);
        h = lex_min(Head{lo[0], hi[0], (int)jj[0]}, Head{lo[1], hi[1], (int)jj[1]});
    }
    v = h.value();
    j = h.j;
}

}  // namespace dbgsom
