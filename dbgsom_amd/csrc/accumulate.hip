// Per-neuron sums of one epoch on gfx950: S_j = sum kw_i x_i, K_j = sum kw_i, a_j = hits,
// E_j = sum dist_i, id-indexed and bitwise reproducible.
//
// Replaces (reference dbgsom/BaseSom.py)
//   :488-489    argsort(winners) / unique(return_index)          -> stable counting sort
//   :1028-1055  numba_voronoi_set_centers (numerator/denominator) -> ordered segmented sums
//   :500-503    neuron_activations                                -> histogram counts
//   :1058-1073  numba_quantization_error (serial semantics)       -> ordered segmented sum
//
// HBM-bound: X is streamed exactly once (row gathers of whole contiguous rows, 16 B per lane),
// everything else is O(N) integers or O(chunks * d).  No floating-point atomics: samples are
// bucketed by winner with a stable counting sort (per-workgroup LDS histograms + a column scan),
// each neuron's list is cut into chunks of <= CH rows, one workgroup sums one chunk in list
// order, and a second pass adds a neuron's chunk partials in chunk order.
//
// Weighted form (`sw`, one float64 per row: a row of weight w counts as w copies of that row):
//   S_j = sum w_i kw_i x_i, K_j = sum w_i kw_i, a_j = sum w_i, E_j = sum w_i dist_i.
// The kernels' template parameter WGT: the unweighted kernels are the WGT = false instantiations
// (nothing of the weighted form is in them: `if constexpr`, an empty argument struct) and compile to
// what they were.  a_j is then
// a third scalar partial per chunk (slab rows d + 3 wide), added in list, chunk and group order like
// K and E.  The counting sort is the unweighted one (`order`, the next filtered search's visiting
// order, stays bucketed by winner: rows of weight 0 in a bucket of their own behind the neurons made
// that search fall back to all pairs -- 24 ms against 2.1 at C4 with a third of the rows at 0); a row
// of weight 0 keeps its slot in its neuron's list and is skipped there: never streamed, added to
// nothing, so a neuron that only such rows chose keeps exact zeros.
#include "common.h"

namespace dbgsom {

constexpr int AT = 256;          // threads per workgroup
// samples per histogram / scatter workgroup: a scatter wavefront walks its samples 64 per round, one
// dependent round after the other -- 2048 samples are 32 rounds for one wavefront (scatter_kernel), 8 for
// each of four (scatter4_kernel); a small sample set (C2, a rank's share in strong scaling) gets 512 =
// 8 / 2 rounds and four times the workgroups.  A function of N alone.
static int hs_for(int64_t N) { return N <= 300000 ? 512 : 2048; }
constexpr int CH = 128;          // rows per segmented-sum chunk

struct AccWs {
    int32_t *order;       // N          sample ids, bucketed by winner, stable
    uint32_t *blk;        // nb * M     per-workgroup histograms -> exclusive block offsets
    uint32_t *count;      // M
    uint32_t *seg_start;  // M + 1
    uint32_t *chunk_pre;  // M + 1      exclusive scan of ceil(count / CH)
    double *slab;         // maxchunks * (d + 2)   [partial S | partial K | partial E]
    double *gslab;        // M * finalize_groups(M) * (d + 2): second level of the ordered sum
    uint32_t *ticket;     // "last workgroup" ticket of the fused column / segment scan
    uint32_t *oob;        // nb         per histogram workgroup: one of its winners is outside [0, M)
    int64_t nb, maxchunks;
};

// A small map has few neurons with very many chunk partials each: their ordered sum is split into
// NG consecutive groups summed side by side (then added in group order) so that it fills the
// chip; NG depends on M alone, the grouping on the counts alone -> still bitwise reproducible.
static int finalize_groups(int64_t M) {
    const int64_t g = 512 / (M > 0 ? M : 1);
    return (int)(g < 1 ? 1 : (g > 32 ? 32 : g));
}

// ns = scalar partials per slab row (2, weighted: 3)
static size_t carve(AccWs *w, char *base, int64_t N, int64_t d, int64_t M, int ns = 2) {
    const int HS = hs_for(N);
    const int64_t nb = (N + HS - 1) / HS;
    const int64_t maxchunks = (N + CH - 1) / CH + M;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += align_up(bytes); return o; };
    const size_t o_order = take((size_t)N * 4);
    const size_t o_blk = take((size_t)nb * M * 4);
    const size_t o_count = take((size_t)M * 4);
    const size_t o_seg = take((size_t)(M + 1) * 4);
    const size_t o_chunk = take((size_t)(M + 1) * 4);
    const size_t o_slab = take((size_t)maxchunks * (d + ns) * 8);
    const size_t o_gslab = take((size_t)M * finalize_groups(M) * (d + ns) * 8);
    const size_t o_ticket = take(256);
    const size_t o_oob = take((size_t)nb * 4);
    if (w) {
        w->ticket = (uint32_t *)(base + o_ticket);
        w->oob = (uint32_t *)(base + o_oob);
        w->order = (int32_t *)(base + o_order);
        w->blk = (uint32_t *)(base + o_blk);
        w->count = (uint32_t *)(base + o_count);
        w->seg_start = (uint32_t *)(base + o_seg);
        w->chunk_pre = (uint32_t *)(base + o_chunk);
        w->slab = (double *)(base + o_slab);
        w->gslab = (double *)(base + o_gslab);
        w->nb = nb;
        w->maxchunks = maxchunks;
    }
    return off;
}

size_t accumulate_workspace_bytes(int64_t N, int64_t d, int64_t M) {
    if (N < 0 || d < 1 || M < 1) return 0;
    return carve(nullptr, nullptr, N, d, M);
}

size_t accumulate_weighted_workspace_bytes(int64_t N, int64_t d, int64_t M) {
    if (N < 0 || d < 1 || M < 1) return 0;
    return carve(nullptr, nullptr, N, d, M, 3);
}

// what the weighted instantiations take behind the unweighted kernels' arguments (nothing at all for
// WGT = false: those kernels are the code they were before the weighted form existed)
template <bool WGT> struct WeightArg {};
template <> struct WeightArg<true> {
    const double *sw;          // one weight per row
};


// ---- 1. per-workgroup histogram of winners ---------------------------------------------------
// A winner outside [0, M) is counted nowhere; the workgroup leaves "I saw one" in oob[blockIdx.x], and the last
// workgroup of the scan kernel STORES the status word from these flags: nothing has to clear the word in front of
// the sort (that was a memset of four bytes, a 5 us hole in the stream), and every call gets its own status.
__global__ __launch_bounds__(AT) void hist_kernel(const int64_t *__restrict__ win, int64_t N,
                                                  int M, uint32_t *__restrict__ blk,
                                                  uint32_t *__restrict__ oob,
                                                  uint32_t *__restrict__ ticket, int HS) {
    extern __shared__ uint32_t h[];
    __shared__ uint32_t bad;
    if (blockIdx.x == 0 && threadIdx.x == 0) *ticket = 0u;  // of the scan kernel that follows
    if (threadIdx.x == 0) bad = 0u;
    for (int j = threadIdx.x; j < M; j += AT) h[j] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * HS;
    for (int t = threadIdx.x; t < HS; t += AT) {
        const int64_t i = base + t;
        if (i < N) {
            const int64_t j = win[i];
            if (j >= 0 && j < M) atomicAdd(&h[j], 1u);
            else bad = 1u;
        }
    }
    __syncthreads();
    uint32_t *dst = blk + (size_t)blockIdx.x * M;
    for (int j = threadIdx.x; j < M; j += AT) dst[j] = h[j];
    if (threadIdx.x == 0) oob[blockIdx.x] = bad;
}

// ---- 2. column scan over workgroups: blk -> exclusive offsets, count[j] ----------------------
// A column is nb = N / HS entries long and its prefix is serial: CS_GROUPS threads share it (sum of
// a group of consecutive workgroups each, prefix over the groups in LDS, then every thread rewrites
// its group).  1024 threads per workgroup: 32 columns (one 128-byte line per row of the table) x 32 groups --
// a thread's share of a column is nb / 32 entries.  Up to CS_BATCH of them are ONE batch of loads and stay in
// registers for the rewrite (C4, C3: 489 rows, 16 per thread -- two memory round trips where 8 groups and two passes
// of 8-entry batches made sixteen); longer shares walk twice in batches of 8.
constexpr int CS_COLS = 32, CS_GROUPS = 32, CS_BATCH = 16;
constexpr int CS_THREADS = CS_COLS * CS_GROUPS;
__device__ __forceinline__ void colscan_body(uint32_t *__restrict__ blk, int64_t nb, int M,
                                             uint32_t *__restrict__ count) {
    __shared__ uint32_t part[CS_GROUPS][CS_COLS];
    const int c = threadIdx.x % CS_COLS, g = threadIdx.x / CS_COLS;
    const int j = blockIdx.x * CS_COLS + c;
    const int jc = min(j, M - 1);   // (columns behind M: loads clamped, nothing stored)
    const int64_t len = (nb + CS_GROUPS - 1) / CS_GROUPS;
    const int64_t b0 = min(nb, (int64_t)g * len), b1 = min(nb, b0 + len);
    const bool one = len <= CS_BATCH;   // (uniform)
    uint32_t sum = 0;
    uint32_t v[CS_BATCH];
    if (one) {
#pragma unroll
        for (int u = 0; u < CS_BATCH; ++u) v[u] = blk[(size_t)min(b0 + u, nb - 1) * M + jc];
#pragma unroll
        for (int u = 0; u < CS_BATCH; ++u) {
            v[u] = (b0 + u < b1) ? v[u] : 0u;
            sum += v[u];
        }
    } else if (j < M) {
        int64_t b = b0;
        for (; b + 8 <= b1; b += 8) {  // 8 independent loads in flight
            uint32_t x[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) x[u] = blk[(size_t)(b + u) * M + j];
#pragma unroll
            for (int u = 0; u < 8; ++u) sum += x[u];
        }
        for (; b < b1; ++b) sum += blk[(size_t)b * M + j];
    }
    part[g][c] = sum;
    __syncthreads();
    uint32_t run = 0;
#pragma unroll
    for (int u = 0; u < CS_GROUPS; ++u) {   // (every read issued, the groups in front selected)
        const uint32_t x = part[u][c];
        run += (u < g) ? x : 0u;
    }
    if (j >= M) return;
    if (g == CS_GROUPS - 1) count[j] = run + sum;
    if (one) {
#pragma unroll
        for (int u = 0; u < CS_BATCH; ++u) {
            if (b0 + u < b1) blk[(size_t)(b0 + u) * M + j] = run;
            run += v[u];
        }
        return;
    }
    int64_t b = b0;
    for (; b + 8 <= b1; b += 8) {
        uint32_t x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = blk[(size_t)(b + u) * M + j];
#pragma unroll
        for (int u = 0; u < 8; ++u) { blk[(size_t)(b + u) * M + j] = run; run += x[u]; }
    }
    for (; b < b1; ++b) {
        const uint32_t x = blk[(size_t)b * M + j];
        blk[(size_t)b * M + j] = run;
        run += x;
    }
}

// ---- 3. exclusive scans over the M neurons (one workgroup of NTHR threads) ----------------------
// A thread's range of neurons is SS_BATCH counts at most on any map the library takes (one batch of loads, kept
// for the second walk); longer ranges walk the table twice.
constexpr int SS_BATCH = 16;
template <int NTHR>
__device__ __forceinline__ void segscan_body(const uint32_t *__restrict__ count, int M,
                                             uint32_t *__restrict__ seg_start,
                                             uint32_t *__restrict__ chunk_pre) {
    constexpr int NWAVE = NTHR / 64;
    __shared__ uint32_t wa[NWAVE], wb[NWAVE];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int per = (M + NTHR - 1) / NTHR;
    const int lo = min(M, t * per), hi = min(M, lo + per);
    const bool one = per <= SS_BATCH;   // (uniform)
    uint32_t cv[SS_BATCH];
    uint32_t a = 0, b = 0;
    if (one) {
#pragma unroll
        for (int u = 0; u < SS_BATCH; ++u) cv[u] = count[min(lo + u, M - 1)];
#pragma unroll
        for (int u = 0; u < SS_BATCH; ++u) {
            cv[u] = (lo + u < hi) ? cv[u] : 0u;
            a += cv[u]; b += (cv[u] + CH - 1) / CH;
        }
    } else {
        for (int j = lo; j < hi; ++j) { a += count[j]; b += (count[j] + CH - 1) / CH; }
    }
    uint32_t ia = a, ib = b;  // inclusive scan over the wavefront, then over the wavefronts
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t va = __shfl_up(ia, off, 64), vb = __shfl_up(ib, off, 64);
        if (lane >= off) { ia += va; ib += vb; }
    }
    if (lane == 63) { wa[wv] = ia; wb[wv] = ib; }
    __syncthreads();
    uint32_t pa = 0, pb = 0;
#pragma unroll
    for (int u = 0; u < NWAVE; ++u) {
        const uint32_t xa = wa[u], xb = wb[u];
        pa += (u < wv) ? xa : 0u; pb += (u < wv) ? xb : 0u;
    }
    if (t == NTHR - 1) { seg_start[M] = pa + ia; chunk_pre[M] = pb + ib; }
    a = pa + ia - a; b = pb + ib - b;  // exclusive prefix of this thread's range
    if (one) {
#pragma unroll
        for (int u = 0; u < SS_BATCH; ++u) {
            if (lo + u < hi) { seg_start[lo + u] = a; chunk_pre[lo + u] = b; }
            a += cv[u]; b += (cv[u] + CH - 1) / CH;
        }
        return;
    }
    for (int j = lo; j < hi; ++j) {
        seg_start[j] = a; chunk_pre[j] = b;
        a += count[j]; b += (count[j] + CH - 1) / CH;
    }
}

// column scan (2.) and, in the workgroup that finishes last, the scans over the neurons (3.): they
// need every column's count, and a kernel of their own is one 5 us launch more per sort.  The same workgroup
// stores the status word from the histogram workgroups' flags (hist_kernel).
__global__ __launch_bounds__(CS_THREADS) void scan_kernel(uint32_t *__restrict__ blk, int64_t nb, int M,
                                                         uint32_t *__restrict__ count,
                                                         uint32_t *__restrict__ seg_start,
                                                         uint32_t *__restrict__ chunk_pre,
                                                         uint32_t *__restrict__ ticket,
                                                         const uint32_t *__restrict__ oob,
                                                         int32_t *__restrict__ status) {
    colscan_body(blk, nb, M, count);
    if (!last_workgroup_done(ticket, gridDim.x)) return;
    uint32_t any = 0;
    if (status) {
        for (int64_t b0 = 0; b0 < nb; b0 += 4 * CS_THREADS) {
            uint32_t f[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) f[u] = oob[min(b0 + u * CS_THREADS + threadIdx.x, nb - 1)];
#pragma unroll
            for (int u = 0; u < 4; ++u) any |= f[u];   // (a clamped load repeats the last flag: the OR is the same)
        }
    }
    segscan_body<CS_THREADS>(count, M, seg_start, chunk_pre);
    const int bad = __syncthreads_or((int)any);
    if (status && threadIdx.x == 0) *status = bad ? 1 : 0;
}

// ---- 4. stable scatter of sample ids into their neuron's segment -----------------------------
// One wavefront per workgroup of HS samples, 64 per round in sample order.  The rank of a sample
// among the lanes holding the same winner comes from ballots over the bits of the key (peers =
// lanes that agree in every bit), the first of them moves the neuron's write position on: no
// search through the round's keys, no barrier between wavefronts.
constexpr int SCW = 64;
template <int HS>
__global__ __launch_bounds__(SCW) void scatter_kernel(const int64_t *__restrict__ win, int64_t N,
                                                      int M, int nbits,
                                                      const uint32_t *__restrict__ blk,
                                                      const uint32_t *__restrict__ seg_start,
                                                      int32_t *__restrict__ order) {
    extern __shared__ uint32_t cnt[];  // M running write positions of this workgroup
    constexpr int R = HS / SCW;
    const int lane = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * HS;
    int keys[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {  // all of the workgroup's keys are in flight at once
        const int64_t i = base + r * SCW + lane;
        int64_t j = -1;
        if (i < N) j = win[i];
        keys[r] = (j >= 0 && j < M) ? (int)j : -1;
    }
    const uint32_t *off = blk + (size_t)blockIdx.x * M;
#pragma unroll 8
    for (int j = lane; j < M; j += SCW) cnt[j] = seg_start[j] + off[j];
    __syncthreads();
    const uint64_t lt = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int key = keys[r];
        uint64_t peers = __builtin_amdgcn_ballot_w64(key >= 0);
        for (int b = 0; b < nbits; ++b) {
            const bool bit = (key >> b) & 1;
            const uint64_t m = __builtin_amdgcn_ballot_w64(bit);
            peers &= bit ? m : ~m;
        }
        const uint64_t before = peers & lt;
        if (key >= 0) order[cnt[key] + (uint32_t)__popcll(before)] = (int32_t)(base + r * SCW + lane);
        __syncthreads();  // every position of this round has been read from cnt
        if (key >= 0 && before == 0) cnt[key] += (uint32_t)__popcll(peers);  // one lane per key
        __syncthreads();
    }
}

// Four wavefronts per workgroup of HS samples: wavefront w takes the w-th quarter, in sample order, with running
// write positions of its OWN in LDS (cnt[w][.]) -- HS / 256 dependent rounds instead of HS / 64, and no workgroup
// barrier inside them: the LDS operations of one wavefront complete in program order, so the round's reads of
// cnt[w][key] are served before its adds, and those before the next round's reads.
// A first pass counts every wavefront's keys (integer LDS atomics: any order, the same counts); wavefront w then
// starts key k at seg_start[k] + this workgroup's block offset + the counts of the wavefronts in front of it: the
// order stays the stable one by (winner, row).
// 4 M counters = 16 M bytes of LDS: maps above SC4_MAX_M (where that leaves fewer than two workgroups per CU) keep
// the one-wavefront kernel.
constexpr int SC4 = 4;
constexpr int SC4_MAX_M = 160 * 1024 / 2 / (SC4 * 4);
template <int HS>
__global__ __launch_bounds__(SC4 * SCW) void scatter4_kernel(const int64_t *__restrict__ win, int64_t N,
                                                             int M, int nbits,
                                                             const uint32_t *__restrict__ blk,
                                                             const uint32_t *__restrict__ seg_start,
                                                             int32_t *__restrict__ order) {
    extern __shared__ uint32_t cnt[];  // [SC4][M]
    constexpr int Q = HS / SC4, R = Q / SCW;
    const int t = threadIdx.x, lane = t & 63;
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
    const int64_t base = (int64_t)blockIdx.x * HS + wv * Q;
    int keys[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {  // all of the wavefront's keys are in flight at once
        const int64_t i = base + r * SCW + lane;
        int64_t j = -1;
        if (i < N) j = win[i];
        keys[r] = (j >= 0 && j < M) ? (int)j : -1;
    }
    for (int j = t; j < SC4 * M; j += SC4 * SCW) cnt[j] = 0u;
    __syncthreads();
    uint32_t *mine = cnt + (size_t)wv * M;
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (keys[r] >= 0) atomicAdd(&mine[keys[r]], 1u);
    __syncthreads();
    const uint32_t *off = blk + (size_t)blockIdx.x * M;
    for (int j0 = 0; j0 < M; j0 += 4 * SC4 * SCW) {
        uint32_t p[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int jc = min(j0 + u * SC4 * SCW + t, M - 1);
            p[u] = seg_start[jc] + off[jc];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + u * SC4 * SCW + t;
            if (j < M) {
                uint32_t run = p[u];
#pragma unroll
                for (int w = 0; w < SC4; ++w) {
                    const uint32_t c = cnt[(size_t)w * M + j];
                    cnt[(size_t)w * M + j] = run;
                    run += c;
                }
            }
        }
    }
    __syncthreads();
    const uint64_t lt = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int key = keys[r];
        uint64_t peers = __builtin_amdgcn_ballot_w64(key >= 0);
        for (int b = 0; b < nbits; ++b) {
            const bool bit = (key >> b) & 1;
            const uint64_t m = __builtin_amdgcn_ballot_w64(bit);
            peers &= bit ? m : ~m;
        }
        const uint64_t before = peers & lt;
        if (key >= 0) order[mine[key] + (uint32_t)__popcll(before)] = (int32_t)(base + r * SCW + lane);
        __builtin_amdgcn_wave_barrier();   // (program order of the LDS read above and the add below)
        if (key >= 0 && before == 0) mine[key] += (uint32_t)__popcll(peers);  // one lane per key
        __builtin_amdgcn_wave_barrier();
    }
}
// (non-temporal: every row is read exactly once by this kernel, 16 bytes per lane and whole cache lines per
//  wavefront instruction -- streamed past the caches, segsum_kernel's 3.4 GB at C4 take 0.57 instead of 0.64 ms)
template <typename XT, int VEC>
__device__ __forceinline__ void load_vec(const XT *__restrict__ src, double (&v)[VEC]) {
    if constexpr (sizeof(XT) == 4 && VEC == 4) {
        typedef float f4_t __attribute__((ext_vector_type(4)));
        const f4_t t4 = __builtin_nontemporal_load(reinterpret_cast<const f4_t *>(src));
        v[0] = t4.x; v[1] = t4.y; v[2] = t4.z; v[3] = t4.w;
    } else if constexpr (sizeof(XT) == 8 && VEC == 2) {
        typedef double d2_t __attribute__((ext_vector_type(2)));
        const d2_t t2 = __builtin_nontemporal_load(reinterpret_cast<const d2_t *>(src));
        v[0] = t2.x; v[1] = t2.y;
    } else if constexpr (sizeof(XT) == 2 && VEC == 8) {
        typedef unsigned u4_t __attribute__((ext_vector_type(4)));
        const u4_t a = __builtin_nontemporal_load(reinterpret_cast<const u4_t *>(src));
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[2 * e] = (double)__uint_as_float(a[e] << 16);
            v[2 * e + 1] = (double)__uint_as_float(a[e] & 0xffff0000u);
        }
    } else {
        static_assert(VEC == 1, "unsupported vector width");
        v[0] = widen(src[0]);
    }
}

// ---- 5. one workgroup sums one chunk (<= CH rows of one neuron) in list order ----------------
// (WGT: per row the factor w kw on the x-sum and K -- one rounded product --, w dist on E, and the
//  third scalar partial sum w)
template <typename XT, int VEC, bool WGT>
__global__ __launch_bounds__(AT) void segsum_kernel(
    const XT *__restrict__ X, int d, int64_t ldx, const int32_t *__restrict__ order,
    const double *__restrict__ kw, double gamma, const double *__restrict__ dist,
    const uint32_t *__restrict__ seg_start, const uint32_t *__restrict__ count,
    const uint32_t *__restrict__ chunk_pre, int M, double *__restrict__ slab, WeightArg<WGT> wa) {
    constexpr int NS = WGT ? 3 : 2;   // scalar partials behind the d columns of a slab row
    __shared__ int32_t rows_s[CH];
    __shared__ double kw_s[CH];
    __shared__ double dist_s[CH];
    __shared__ double sw_s[WGT ? CH : 1];
    __shared__ double red[AT * VEC];
    __shared__ uint32_t info[3];
    const int tid = threadIdx.x;
    const uint32_t c = blockIdx.x;
    if (c >= chunk_pre[M]) return;  // uniform per workgroup
    if (tid == 0) {
        int lo = 0, hi = M;  // last j with chunk_pre[j] <= c
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (chunk_pre[mid] <= c) lo = mid; else hi = mid;
        }
        const uint32_t begin = seg_start[lo] + (c - chunk_pre[lo]) * CH;
        const uint32_t end = min(begin + (uint32_t)CH, seg_start[lo] + count[lo]);
        info[0] = begin; info[1] = end - begin;
    }
    __syncthreads();
    const uint32_t begin = info[0];
    const int n = (int)info[1];
    if (tid < n) {
        const int32_t r = order[begin + tid];
        rows_s[tid] = r;
        const double dd = dist[r];
        // kw == nullptr: the sample kernel of BaseSom._calculate_exp_similarity (BaseSom.py:533-538)
        // on the fly, the arithmetic of exp_similarity_kernel (bmu.hip)
        const double h = kw ? kw[r] : 1.0 - sqrt(1.0 - exp(-gamma * (dd * dd)));
        if constexpr (WGT) {
            const double w = wa.sw[r];
            sw_s[tid] = w;
            kw_s[tid] = __dmul_rn(w, h);
            dist_s[tid] = __dmul_rn(w, dd);
        } else {
            kw_s[tid] = h;
            dist_s[tid] = dd;
        }
    }
    __syncthreads();
    double *out = slab + (size_t)c * (d + NS);
    if (tid == AT - 1) {  // the scalar partials, in list order
        double sk = 0.0, se = 0.0;
        for (int p = 0; p < n; ++p) { sk += kw_s[p]; se += dist_s[p]; }
        out[d] = sk;
        out[d + 1] = se;
        if constexpr (WGT) {
            double sa = 0.0;
            for (int p = 0; p < n; ++p) sa += sw_s[p];
            out[d + 2] = sa;
        }
    }
    const int Q = d / VEC;  // column groups (VEC divides d by construction)
    if (Q >= AT) {
        for (int q = tid; q < Q; q += AT) {
            double acc[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e] = 0.0;
#pragma unroll 4
            for (int p = 0; p < n; ++p) {
                if constexpr (WGT) { if (sw_s[p] == 0.0) continue; }   // (weight 0: not streamed)
                const XT *src = X + (int64_t)rows_s[p] * ldx + (int64_t)q * VEC;
                const double w = kw_s[p];
                double v[VEC];
                load_vec<XT, VEC>(src, v);
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[e] += w * v[e];
            }
#pragma unroll
            for (int e = 0; e < VEC; ++e) out[q * VEC + e] = acc[e];
        }
    } else {
        const int RL = AT / Q;  // row lanes working side by side on the same column group
        const int rl = tid / Q, q = tid - rl * Q;
        double acc[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] = 0.0;
        if (rl < RL) {
#pragma unroll 4
            for (int p = rl; p < n; p += RL) {
                if constexpr (WGT) { if (sw_s[p] == 0.0) continue; }
                const XT *src = X + (int64_t)rows_s[p] * ldx + (int64_t)q * VEC;
                const double w = kw_s[p];
                double v[VEC];
                load_vec<XT, VEC>(src, v);
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[e] += w * v[e];
            }
#pragma unroll
            for (int e = 0; e < VEC; ++e) red[(rl * Q + q) * VEC + e] = acc[e];
        }
        __syncthreads();
        if (rl == 0) {  // row lanes are added in lane order
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                double s = red[q * VEC + e];
                for (int u = 1; u < RL; ++u) s += red[(u * Q + q) * VEC + e];
                out[q * VEC + e] = s;
            }
        }
    }
}
// ---- 6. add each neuron's chunk partials in chunk order --------------------------------------
// (WGT: a_j is the ordered sum of the chunks' third scalar partial instead of the integer count)
template <bool WGT>
__global__ __launch_bounds__(AT) void finalize_kernel(const double *__restrict__ slab, int d,
                                                      int M, const uint32_t *__restrict__ count,
                                                      const uint32_t *__restrict__ chunk_pre,
                                                      int NG, double *__restrict__ gslab,
                                                      double *__restrict__ sums,
                                                      const int32_t *__restrict__ status,
                                                      double *__restrict__ status_f64) {
    constexpr int NS = WGT ? 3 : 2;
    const int j = blockIdx.x, g = blockIdx.y;
    if (status_f64 && j == 0 && g == 0 && blockIdx.z == 0 && threadIdx.x == 0)
        status_f64[0] = status[0] ? 1.0 : 0.0;   // the flag rides behind the sums in the all-reduce buffer
    const uint32_t b0 = chunk_pre[j], b1 = chunk_pre[j + 1];
    const uint32_t per = (b1 - b0 + NG - 1) / NG;  // chunks per group
    const uint32_t c0 = min(b1, b0 + g * per), c1 = min(b1, c0 + per);
    double *S = sums + (size_t)j * d;
    double *Kp = sums + (size_t)M * d, *ap = Kp + M, *Ep = ap + M;
    // (the column blocks of a neuron are separate workgroups, gridDim.z of them: one short chain
    // per thread instead of four one after the other)
    for (int col = threadIdx.x + AT * blockIdx.z; col < d + NS; col += AT * gridDim.z) {
        double s = 0.0;
        uint32_t c = c0;
        for (; c + 8 <= c1; c += 8) {  // loads batched, additions still in chunk order
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = slab[(size_t)(c + u) * (d + NS) + col];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
        for (; c < c1; ++c) s += slab[(size_t)c * (d + NS) + col];
        if (NG > 1) gslab[((size_t)j * NG + g) * (d + NS) + col] = s;
        else if (col < d) S[col] = s;
        else if (col == d) Kp[j] = s;
        else if (!WGT || col == d + 1) Ep[j] = s;
        else ap[j] = s;
    }
    if constexpr (!WGT) {
        if (threadIdx.x == 0 && g == 0 && blockIdx.z == 0) ap[j] = (double)count[j];
    }
}

// second level (NG > 1): the NG group sums of a neuron in group order
template <bool WGT>
__global__ __launch_bounds__(AT) void finalize_groups_kernel(const double *__restrict__ gslab, int d,
                                                             int M, int NG,
                                                             double *__restrict__ sums) {
    constexpr int NS = WGT ? 3 : 2;
    const int j = blockIdx.x;
    double *S = sums + (size_t)j * d;
    double *Kp = sums + (size_t)M * d, *Ep = Kp + 2 * (size_t)M;
    for (int col = threadIdx.x; col < d + NS; col += AT) {
        double s = 0.0;
        for (int g = 0; g < NG; ++g) s += gslab[((size_t)j * NG + g) * (d + NS) + col];
        if (col < d) S[col] = s;
        else if (col == d) Kp[j] = s;
        else if (!WGT || col == d + 1) Ep[j] = s;
        else Kp[(size_t)M + j] = s;
    }
}

static int key_bits(int64_t M) {  // bits that tell the keys 0 .. M - 1 apart
    int b = 0;
    while (((int64_t)1 << b) < M) ++b;
    return b;
}

// Stable bucket order of the samples by winner, on its own (the filtered BMU search visits the
// samples in this order).  `ws` needs bucket_sort_workspace_bytes(N, M); `order` gets N int32.
size_t bucket_sort_workspace_bytes(int64_t N, int64_t M) {
    const int HS = hs_for(N);
    const int64_t nb = (N + HS - 1) / HS;
    return align_up((size_t)nb * M * 4) + align_up((size_t)M * 4) + 2 * align_up((size_t)(M + 1) * 4) + 256 +
           align_up((size_t)nb * 4);   // (blk, count, seg_start, chunk_pre, ticket, the histogram workgroups' flags)
}

// where launch_bucket_sort leaves the exclusive segment starts (M + 1 entries) in its workspace
const uint32_t *bucket_sort_seg_start(const void *ws, int64_t N, int64_t M) {
    const int HS = hs_for(N);
    const int64_t nb = (N + HS - 1) / HS;
    return reinterpret_cast<const uint32_t *>((const char *)ws + align_up((size_t)nb * M * 4) + align_up((size_t)M * 4));
}

// all three tables launch_bucket_sort leaves in its workspace (M, M + 1 and M + 1 entries), and the chunk length
// chunk_pre is cut by: what a sibling of segsum_kernel in another source needs (masked_fit.hip)
void bucket_sort_tables(const void *ws, int64_t N, int64_t M, const uint32_t **count, const uint32_t **seg_start,
                        const uint32_t **chunk_pre) {
    const int HS = hs_for(N);
    const int64_t nb = (N + HS - 1) / HS;
    const char *base = (const char *)ws + align_up((size_t)nb * M * 4);
    *count = reinterpret_cast<const uint32_t *>(base);
    base += align_up((size_t)M * 4);
    *seg_start = reinterpret_cast<const uint32_t *>(base);
    base += align_up((size_t)(M + 1) * 4);
    *chunk_pre = reinterpret_cast<const uint32_t *>(base);
}
int accumulate_chunk_rows() { return CH; }

template <int HS>
static int launch_scatter4(const int64_t *idx, int64_t N, int Mi, int64_t nb, const uint32_t *blk,
                           const uint32_t *seg_start, int32_t *order, hipStream_t s) {
    static bool attr_set = false;   // (16 M bytes of LDS: above the default limit from M = 4097 on)
    if (!attr_set) {
        DBGSOM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&scatter4_kernel<HS>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, SC4_MAX_M * SC4 * 4));
        attr_set = true;
    }
    hipLaunchKernelGGL(scatter4_kernel<HS>, dim3((unsigned)nb), dim3(SC4 * SCW), (size_t)Mi * SC4 * 4, s, idx, N, Mi,
                       key_bits(Mi), blk, seg_start, order);
    return DBGSOM_OK;
}

static int launch_scatter(const int64_t *idx, int64_t N, int Mi, int64_t nb, const uint32_t *blk,
                          const uint32_t *seg_start, int32_t *order, hipStream_t s) {
    if (Mi <= SC4_MAX_M)
        return hs_for(N) == 512 ? launch_scatter4<512>(idx, N, Mi, nb, blk, seg_start, order, s)
                                : launch_scatter4<2048>(idx, N, Mi, nb, blk, seg_start, order, s);
    if (hs_for(N) == 512)
        hipLaunchKernelGGL(scatter_kernel<512>, dim3((unsigned)nb), dim3(SCW), (size_t)Mi * 4, s, idx, N, Mi,
                           key_bits(Mi), blk, seg_start, order);
    else
        hipLaunchKernelGGL(scatter_kernel<2048>, dim3((unsigned)nb), dim3(SCW), (size_t)Mi * 4, s, idx, N, Mi,
                           key_bits(Mi), blk, seg_start, order);
    return DBGSOM_OK;
}

int launch_bucket_sort(const int64_t *idx, int64_t N, int64_t M, int32_t *order, void *ws,
                       hipStream_t s) {
    const int HS = hs_for(N);
    const int64_t nb = (N + HS - 1) / HS;
    char *base = (char *)ws;
    uint32_t *blk = (uint32_t *)base;
    base += align_up((size_t)nb * M * 4);
    uint32_t *count = (uint32_t *)base;
    base += align_up((size_t)M * 4);
    uint32_t *seg_start = (uint32_t *)base;
    base += align_up((size_t)(M + 1) * 4);
    uint32_t *chunk_pre = (uint32_t *)base;
    base += align_up((size_t)(M + 1) * 4);
    uint32_t *ticket = (uint32_t *)base;
    base += 256;
    uint32_t *oob = (uint32_t *)base;
    const int Mi = (int)M;
    hipLaunchKernelGGL(hist_kernel, dim3((unsigned)nb), dim3(AT), (size_t)M * 4, s, idx, N, Mi, blk, oob, ticket, HS);
    hipLaunchKernelGGL(scan_kernel, dim3((unsigned)((M + CS_COLS - 1) / CS_COLS)), dim3(CS_THREADS), 0, s, blk, nb, Mi,
                       count, seg_start, chunk_pre, ticket, (const uint32_t *)oob, (int32_t *)nullptr);
    const int rc = launch_scatter(idx, N, Mi, nb, blk, seg_start, order, s);
    if (rc != DBGSOM_OK) return rc;
    return launch_status("bucket sort kernels");
}

// ---------------------------------------------------------------------------------------------
static int accumulate_impl(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx,
                           const int64_t *idx, const double *kw, double gamma, const double *dist, int64_t M,
                           double *sums, int32_t *status, bool status_behind_sums, void *ws,
                           size_t ws_bytes, hipStream_t s, const double *sw = nullptr, const CsrView *csr = nullptr) {
    DBGSOM_REQUIRE(valid_dtype(x_dtype), "x_dtype must be DBGSOM_F32/F64/BF16");
    DBGSOM_REQUIRE(N >= 0 && N < 0x7fffffff && d >= 1 && d <= 0x7ffffff0 && ldx >= d, "bad sample shape");
    DBGSOM_REQUIRE(M >= 1 && M <= DBGSOM_MAX_PROTOTYPES, "M outside [1, DBGSOM_MAX_PROTOTYPES]");
    DBGSOM_REQUIRE(sums, "null sums");
    DBGSOM_REQUIRE(!status_behind_sums || status, "the status flag is needed behind the sums");
    if (N == 0) {   // (no sort, nobody to store the status word)
        if (status) DBGSOM_HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int32_t), s));
        DBGSOM_HIP_CHECK(hipMemsetAsync(sums, 0, (size_t)(M * (d + 3) + (status_behind_sums ? 1 : 0)) * sizeof(double), s));
        return DBGSOM_OK;
    }
    DBGSOM_REQUIRE((X || csr) && idx && dist && ws, "null pointer");
    DBGSOM_REQUIRE(is_aligned(ws, 256), "workspace must be 256-byte aligned");
    const size_t need = sw ? accumulate_weighted_workspace_bytes(N, d, M) : accumulate_workspace_bytes(N, d, M);
    if (ws_bytes < need) {
        set_error("dbgsom_accumulate: workspace too small (%zu < %zu)", ws_bytes, need);
        return DBGSOM_ENOMEM;
    }
    AccWs w;
    carve(&w, (char *)ws, N, d, M, sw ? 3 : 2);
    const int Mi = (int)M, di = (int)d;

    hipLaunchKernelGGL(hist_kernel, dim3((unsigned)w.nb), dim3(AT), (size_t)M * 4, s, idx, N, Mi,
                       w.blk, w.oob, w.ticket, hs_for(N));
    hipLaunchKernelGGL(scan_kernel, dim3((unsigned)((M + CS_COLS - 1) / CS_COLS)), dim3(CS_THREADS), 0, s, w.blk, w.nb,
                       Mi, w.count, w.seg_start, w.chunk_pre, w.ticket, (const uint32_t *)w.oob, status);
    {
        const int rc = launch_scatter(idx, N, Mi, w.nb, w.blk, w.seg_start, w.order, s);
        if (rc != DBGSOM_OK) return rc;
    }

    const size_t xe = dtype_size(x_dtype);
    const bool al16 = is_aligned(X, 16) && ((ldx * xe) % 16 == 0);
    dim3 grid((unsigned)w.maxchunks), block(AT);
#define DBGSOM_SEGSUM(XT, V)                                                                    \
    do {                                                                                        \
        if (sw)                                                                                 \
            hipLaunchKernelGGL((segsum_kernel<XT, V, true>), grid, block, 0, s, (const XT *)X, di, ldx, w.order, \
                               kw, gamma, dist, w.seg_start, w.count, w.chunk_pre, Mi, w.slab,   \
                               WeightArg<true>{sw});                                    \
        else                                                                                    \
            hipLaunchKernelGGL((segsum_kernel<XT, V, false>), grid, block, 0, s, (const XT *)X, di, ldx, w.order, \
                               kw, gamma, dist, w.seg_start, w.count, w.chunk_pre, Mi, w.slab,   \
                               WeightArg<false>{});                                              \
    } while (0)
    if (csr) {
        // CSR samples: the chunk kernel of csr.hip writes the same slab rows; everything around it is shared
        const int rc = launch_segsum_csr(*csr, x_dtype, d, w.order, kw, gamma, dist, w.seg_start, w.count, w.chunk_pre, M,
                                         w.slab, sw, w.maxchunks, s);
        if (rc != DBGSOM_OK) return rc;
    } else if (x_dtype == DBGSOM_F32) {
        if (al16 && d % 4 == 0) DBGSOM_SEGSUM(float, 4); else DBGSOM_SEGSUM(float, 1);
    } else if (x_dtype == DBGSOM_F64) {
        if (al16 && d % 2 == 0) DBGSOM_SEGSUM(double, 2); else DBGSOM_SEGSUM(double, 1);
    } else {
        if (al16 && d % 8 == 0) DBGSOM_SEGSUM(bf16_t, 8); else DBGSOM_SEGSUM(bf16_t, 1);
    }
#undef DBGSOM_SEGSUM
    const int NG = finalize_groups(M);
    if (sw) {
        const unsigned col_blocks = (unsigned)((d + 3 + AT - 1) / AT < 8 ? (d + 3 + AT - 1) / AT : 8);
        hipLaunchKernelGGL(finalize_kernel<true>, dim3((unsigned)M, (unsigned)NG, col_blocks), dim3(AT), 0, s, w.slab, di, Mi,
                           w.count, w.chunk_pre, NG, w.gslab, sums, (const int32_t *)status,
                           status_behind_sums ? sums + (size_t)M * (d + 3) : (double *)nullptr);
        if (NG > 1)
            hipLaunchKernelGGL(finalize_groups_kernel<true>, dim3((unsigned)M), dim3(AT), 0, s, w.gslab, di, Mi, NG,
                               sums);
        return launch_status("weighted accumulate kernels");
    }
    const unsigned col_blocks = (unsigned)((d + 2 + AT - 1) / AT < 8 ? (d + 2 + AT - 1) / AT : 8);
    hipLaunchKernelGGL(finalize_kernel<false>, dim3((unsigned)M, (unsigned)NG, col_blocks), dim3(AT), 0, s, w.slab, di, Mi,
                       w.count, w.chunk_pre, NG, w.gslab, sums, (const int32_t *)status,
                       status_behind_sums ? sums + (size_t)M * (d + 3) : (double *)nullptr);
    if (NG > 1)
        hipLaunchKernelGGL(finalize_groups_kernel<false>, dim3((unsigned)M), dim3(AT), 0, s, w.gslab, di, Mi, NG,
                           sums);
    return launch_status("accumulate kernels");
}

int launch_accumulate(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx,
                      const int64_t *idx, const double *kw, const double *dist, int64_t M,
                      double *sums, int32_t *status, void *ws, size_t ws_bytes, hipStream_t s) {
    DBGSOM_REQUIRE(N == 0 || kw, "null sample weights");
    return accumulate_impl(X, x_dtype, N, d, ldx, idx, kw, 0.0, dist, M, sums, status, false, ws, ws_bytes, s);
}

int launch_accumulate_epoch(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx,
                            const int64_t *idx, double gamma, const double *dist, int64_t M,
                            double *sums, int32_t *status, void *ws, size_t ws_bytes, hipStream_t s) {
    return accumulate_impl(X, x_dtype, N, d, ldx, idx, nullptr, gamma, dist, M, sums, status, true, ws, ws_bytes, s);
}

// the weighted forms: `sw` = one weight per row (finite, >= 0: the caller has checked); workspace of
// accumulate_weighted_workspace_bytes
int launch_accumulate_weighted(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx,
                               const int64_t *idx, const double *kw, const double *sw, const double *dist, int64_t M,
                               double *sums, int32_t *status, void *ws, size_t ws_bytes, hipStream_t s) {
    DBGSOM_REQUIRE(N == 0 || (kw && sw), "null sample weights");
    return accumulate_impl(X, x_dtype, N, d, ldx, idx, kw, 0.0, dist, M, sums, status, false, ws, ws_bytes, s, sw);
}

int launch_accumulate_epoch_weighted(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx,
                                     const int64_t *idx, double gamma, const double *sw, const double *dist, int64_t M,
                                     double *sums, int32_t *status, void *ws, size_t ws_bytes, hipStream_t s) {
    DBGSOM_REQUIRE(N == 0 || sw, "null sample weights");
    return accumulate_impl(X, x_dtype, N, d, ldx, idx, nullptr, gamma, dist, M, sums, status, true, ws, ws_bytes, s, sw);
}

int launch_accumulate_csr(const CsrView &x, int x_dtype, int64_t N, int64_t d, const int64_t *idx, const double *kw,
                          double gamma, const double *sw, const double *dist, int64_t M, double *sums,
                          int32_t *status, bool status_behind_sums, void *ws, size_t ws_bytes, hipStream_t s) {
    DBGSOM_REQUIRE(x_dtype == DBGSOM_F32 || x_dtype == DBGSOM_F64, "CSR data must be DBGSOM_F32 or DBGSOM_F64");
    DBGSOM_REQUIRE(N == 0 || x.indptr, "null CSR arrays");
    return accumulate_impl(nullptr, x_dtype, N, d, d, idx, kw, gamma, dist, M, sums, status, status_behind_sums, ws,
                           ws_bytes, s, sw, &x);
}

}  // namespace dbgsom
