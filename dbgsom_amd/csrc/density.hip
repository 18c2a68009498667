// The rows of X within a radius of every prototype on gfx950 (MI355X), at 1 .. DBGSOM_MAX_RADII radii in one pass: the
// all-pairs search read down its columns into integer counts, without the N x M matrix ever leaving the chip's caches.
//
// Per slab of rows, on one stream:
//   1. the squared form of distances.hip: r_ij = max((|x_i|^2 + (-2 <x_i, w_j>)) + |w_j|^2, 0) of slab_rows x M pairs
//      into the workspace, ordinary stores (what launch_kneighbors runs);
//   2. the fold (launch_range_count_cols): counts[j, t] += #{ i : r_ij <= thr[t] }.
// The thresholds are squared values: the host turns a radius rho into the largest float64 t with sqrt(t) <= rho, so that
// r <= t is sqrt(r) <= rho exactly and no root is taken per pair.  A NaN r, or a NaN threshold, counts
// nothing.  The state, M x n_radii int64, is carried from slab to slab and from chunk to chunk; integer adds commute, so
// every partition of the rows and every arrival order gives the same counts.
//
// The fold is one kernel.  The slab is row-major, so a wavefront reads it coalesced only when its lanes own adjacent
// columns: as in topk_cols_partial_kernel the rows are split into segments, one wavefront per (group of 64 columns,
// segment), eight loads in flight per lane; the four wavefronts of a workgroup take adjacent segments of one group.  A
// segment is 64 rows, more (up to 1024) only where that still leaves 4096 wavefronts: nothing but the lane's counters
// is carried down a segment, so its length is chosen for the number of wavefronts alone.
//   range_count_cols_kernel<RB>  RB = n_radii rounded up to 1, 2, 4, 8, 16 or 32; the thresholds past n_radii are NaN.
//       The thresholds are wave-uniform (scalar registers); per loaded value and threshold one compare and one add
//       into a 32-bit counter of the lane, fully unrolled: no indexed register array, nothing in scratch memory.  A
//       wavefront's 64 x n_radii partial counts belong to one contiguous run of the state (the state is row-major, a
//       column's n_radii counts side by side), so they are transposed through LDS, the four wavefronts' counts are
//       summed there, and the workgroup adds them with 64-bit integer vector atomics (device scope), 64 adjacent words
//       per instruction; words that are zero are skipped.
// A two-stage scratch-and-sum was not built: the atomics are at most 1 / 256 of the slab's entries per threshold,
// and they are integer adds whose result is order-free (DESIGN.md 4q has the times).
#include <math.h>

#include <algorithm>

#include "common.h"

namespace dbgsom {

constexpr int RANGE_NT = 256;      // four wavefronts per workgroup
constexpr int RANGE_LOADS = 8;     // loads in flight per lane (segments are multiples of it)
static_assert(RANGE_NT == 256, "the kernel sums the partial counts of four wavefronts");

static int range_instance(int n) { return n <= 1 ? 1 : n <= 2 ? 2 : n <= 4 ? 4 : n <= 8 ? 8 : n <= 16 ? 16 : 32; }
// rows per wavefront: as many as leave RANGE_WAVES wavefronts (four per SIMD of the chip) on the matrix, in multiples of
// the unroll, between 64 and 1024 -- a slab of 8192 x 1024 gets 64-row segments, 2048 wavefronts
constexpr int64_t RANGE_WAVES = 4096, RANGE_SEG_MIN = 64, RANGE_SEG_MAX = 1024;
static int64_t range_segment(int64_t N, int64_t G) {
    const int64_t rows = N * G / RANGE_WAVES / RANGE_LOADS * RANGE_LOADS;
    return std::min(RANGE_SEG_MAX, std::max(RANGE_SEG_MIN, rows));
}

// word p of a wavefront's 64 x n partial counts in LDS: one word of padding per 32, so that neither the lanes' writes
// (n words apart) nor their reads (adjacent) meet on a bank
__device__ __forceinline__ int range_lds_at(int p) { return p + (p >> 5); }

// R: N rows of M squared values, ldr >= M apart.  thr: n thresholds.  counts: M x n, added to.
template <int RB>
__global__ __launch_bounds__(RANGE_NT) void range_count_cols_kernel(const double *__restrict__ R, int N, int M, int64_t ldr,
                                                                    const double *__restrict__ thr, int n, int seg_rows, int G,
                                                                    int64_t S, unsigned long long *__restrict__ counts) {
    __shared__ uint32_t part[RANGE_NT / 64][64 * RB + 2 * RB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // the four wavefronts of a workgroup take adjacent segments of one group of columns: one sum, one run of atomics
    const int g = (int)(blockIdx.x % G);
    const int64_t seg = (int64_t)(blockIdx.x / G) * (RANGE_NT / 64) + wave;
    const bool active = seg < S;   // (wave-uniform; an idle wavefront still writes its zeros and meets the barrier below)
    const int c = 64 * g + lane;
    const bool live = active && c < M;
    // (64-bit row numbers: N may be 2^31 - 1, and the last trip looks past it)
    const int64_t begin = seg * seg_rows, end = active ? std::min<int64_t>(N, (seg + 1) * seg_rows) : begin;

    double t[RB];
    uint32_t cnt[RB];
#pragma unroll
    for (int q = 0; q < RB; ++q) {
        t[q] = (q < n) ? thr[q] : (double)NAN;
        cnt[q] = 0u;
    }
    for (int64_t i0 = begin; i0 < end; i0 += RANGE_LOADS) {
        double r[RANGE_LOADS];
#pragma unroll
        for (int u = 0; u < RANGE_LOADS; ++u) {
            const int64_t i = i0 + u;
            r[u] = (live && i < end) ? R[i * ldr + c] : (double)NAN;   // (NaN passes no threshold)
        }
#pragma unroll
        for (int u = 0; u < RANGE_LOADS; ++u) {
#pragma unroll
            for (int q = 0; q < RB; ++q) cnt[q] += (r[u] <= t[q]) ? 1u : 0u;
        }
    }

    // lane l holds column c's n counts; the state holds them side by side: word l n + q of the wavefront's run
#pragma unroll
    for (int q = 0; q < RB; ++q) {
        if (q < n) part[wave][range_lds_at(lane * n + q)] = cnt[q];
    }
    __syncthreads();
    const int64_t run = (int64_t)64 * g * n, total = (int64_t)M * n;
#pragma unroll
    for (int u = 0; u < RB; ++u) {
        if (u < n && (u & (RANGE_NT / 64 - 1)) == wave) {   // (the runs of 64 words go round the wavefronts)
            const int p = range_lds_at(64 * u + lane);
            const uint32_t v = (part[0][p] + part[1][p]) + (part[2][p] + part[3][p]);   // (<= 4 x 1024 rows)
            if (run + 64 * u + lane < total && v != 0u) atomicAdd(counts + run + 64 * u + lane, (unsigned long long)v);
        }
    }
}

// ---------------------------------------------------------------------------------------------
static int range_check(int64_t M, int n_radii) {
    DBGSOM_REQUIRE(M >= 1 && M <= DBGSOM_MAX_PROTOTYPES, "need 1 <= M <= DBGSOM_MAX_PROTOTYPES");
    DBGSOM_REQUIRE(n_radii >= 1 && n_radii <= DBGSOM_MAX_RADII, "need 1 <= n_radii <= DBGSOM_MAX_RADII");
    return DBGSOM_OK;
}

int launch_range_count_cols(const double *R, int64_t N, int64_t M, int64_t ldr, const double *thr, int n_radii,
                            int64_t *counts, hipStream_t s) {
    DBGSOM_REQUIRE(N >= 0 && N <= 0x7fffffff, "bad sample shape");
    TRY_STATUS(range_check(M, n_radii));
    DBGSOM_REQUIRE(ldr >= M, "ldr must be >= M");
    if (N == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(R && thr && counts, "null pointer");
    DBGSOM_REQUIRE(is_aligned(R, 8) && is_aligned(thr, 8) && is_aligned(counts, 8), "pointers must be 8-byte aligned");
    const int RB = range_instance(n_radii);
    const int64_t G = (M + 63) / 64, seg = range_segment(N, G), S = (N + seg - 1) / seg;
    const int64_t nb = G * ((S + RANGE_NT / 64 - 1) / (RANGE_NT / 64));
    DBGSOM_REQUIRE(nb <= 0x7fffffff, "too many samples for one launch");
    unsigned long long *out = reinterpret_cast<unsigned long long *>(counts);
#define DBGSOM_RANGE(RR)                                                                                                  \
    hipLaunchKernelGGL((range_count_cols_kernel<RR>), dim3((unsigned)nb), dim3(RANGE_NT), 0, s, R, (int)N, (int)M, ldr,  \
                       thr, n_radii, (int)seg, (int)G, S, out)
    switch (RB) {
    case 1: DBGSOM_RANGE(1); break;
    case 2: DBGSOM_RANGE(2); break;
    case 4: DBGSOM_RANGE(4); break;
    case 8: DBGSOM_RANGE(8); break;
    case 16: DBGSOM_RANGE(16); break;
    default: DBGSOM_RANGE(32); break;
    }
#undef DBGSOM_RANGE
    return launch_status("range_count_cols_kernel");
}

// workspace of the slab loop: the slab of launch_kneighbors
size_t range_counts_workspace_bytes(int64_t N, int64_t M, int64_t slab_rows) {
    return kneighbors_workspace_bytes(N, M, slab_rows);
}

static int range_counts_check(int x_dtype, int64_t N, int64_t d, int64_t ldx, int64_t M, int n_radii, int64_t slab_rows) {
    DBGSOM_REQUIRE(valid_dtype(x_dtype), "x_dtype must be DBGSOM_F32/F64/BF16");
    DBGSOM_REQUIRE(N >= 0 && N <= 0x7fffffff && d >= 1 && ldx >= d && d <= 0x7fffffff, "bad sample shape");
    TRY_STATUS(range_check(M, n_radii));
    DBGSOM_REQUIRE(slab_rows >= 0, "slab_rows must be >= 0 (0 = the default)");
    return DBGSOM_OK;
}

// the Euclidean slab loop with the fold behind the product: the N rows are added to a caller's counts
int launch_range_counts_fold(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx, const double *W,
                             int64_t M, const double *ww, const double *thr, int n_radii, int64_t slab_rows, int64_t *counts,
                             void *ws, size_t ws_bytes, hipStream_t s) {
    TRY_STATUS(range_counts_check(x_dtype, N, d, ldx, M, n_radii, slab_rows));
    if (N == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(X && xx && W && ww && thr && counts && ws, "null pointer");
    TRY_STATUS(kneighbors_workspace_check("dbgsom_range_counts", N, M, slab_rows, ws, ws_bytes, 0));
    return euclidean_slabs(X, x_dtype, N, d, ldx, xx, W, M, ww, slab_rows, static_cast<double *>(ws), s,
                           [&](int64_t, int64_t n, const double *slab, int64_t ldr) {
                               return launch_range_count_cols(slab, n, M, ldr, thr, n_radii, counts, s);
                           });
}

int launch_range_counts(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx, const double *W,
                        int64_t M, const double *ww, const double *thr, int n_radii, int64_t slab_rows, int64_t *counts,
                        void *ws, size_t ws_bytes, hipStream_t s) {
    TRY_STATUS(range_counts_check(x_dtype, N, d, ldx, M, n_radii, slab_rows));
    DBGSOM_REQUIRE(counts && (N == 0 || (X && xx && W && ww && thr && ws)), "null pointer");
    DBGSOM_REQUIRE(is_aligned(counts, 8) && is_aligned(thr, 8), "pointers must be 8-byte aligned");
    TRY_STATUS(workspace_check("dbgsom_range_counts", ws_bytes, range_counts_workspace_bytes(N, M, slab_rows)));
    DBGSOM_REQUIRE(N == 0 || is_aligned(ws, 16), "workspace_dev must be 16-byte aligned");
    DBGSOM_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)M * (size_t)n_radii * 8, s));
    return launch_range_counts_fold(X, x_dtype, N, d, ldx, xx, W, M, ww, thr, n_radii, slab_rows, counts, ws, ws_bytes, s);
}

}  // namespace dbgsom

using namespace dbgsom;

extern "C" {

int dbgsom_range_count_cols(const double *R_dev, int64_t N, int64_t M, int64_t ldr, const double *thr_dev, int n_radii,
                            int64_t *counts_dev, void *stream) {
    return launch_range_count_cols(R_dev, N, M, ldr, thr_dev, n_radii, counts_dev, (hipStream_t)stream);
}

size_t dbgsom_range_counts_workspace_bytes(int64_t N, int64_t M, int64_t slab_rows) {
    return range_counts_workspace_bytes(N, M, slab_rows);
}

int dbgsom_range_counts(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx_dev,
                        const double *W_dev, int64_t M, const double *ww_dev, const double *thr_dev, int n_radii,
                        int64_t slab_rows, int64_t *counts_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    return launch_range_counts(X_dev, x_dtype, N, d, ldx, xx_dev, W_dev, M, ww_dev, thr_dev, n_radii, slab_rows, counts_dev,
                               workspace_dev, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
