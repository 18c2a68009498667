// The N x M matrix of distances from every row to every prototype on gfx950 (MI355X): what the all-pairs search
// computes and throws away but for one or two values per row.
//
// Dense rows: siblings of bmu_kernel (bmu.hip, register-staged, any shape) and bmu_dma_kernel (bmu_dma.hip, LDS-DMA
// ring for 16-byte aligned rows with d % 16 == 0).  The product loop of each is kept as it is -- the same
// v_mfma_f64_16x16x4_f64 chain per (row, prototype) pair over the whole feature dimension, so a pair's bits are those
// of the search and of oracle/bmu_chain.c -- and the chunk epilogue is replaced: no running arg-min, no final merge;
//     D_ij = sqrt(max((|x_i|^2 + (-2 <x_i, w_j>)) + |w_j|^2, 0))        (NaN stays NaN)
// is computed for every pair and stored.
//
// Store layout.  Lane (lr, lq) of a wavefront holds, per 16 x 16 tile, ONE row (it * 16 + lr) against the four
// prototypes 4 r + lq, r = 0..3: the four lanes l, l + 16, l + 32, l + 48 together hold 16 consecutive prototypes of
// that row, interleaved.  A 4 x 4 exchange among them (v_permlane32_swap, then v_permlane16_swap: two 2 x 2 block
// transpositions, eight instructions per tile and lane) leaves lane lq with the prototypes 4 lq .. 4 lq + 3: 32
// contiguous bytes per lane, 128 per row and tile, written as two 16-byte stores.  That needs the row base and ldo
// on 16-byte boundaries; where they are not, the values are stored as they lie, 8 bytes each (the four lanes of a
// row still cover 32 contiguous bytes per instruction).  The matrix is never read again here: non-temporal stores.
//
// Squared form (template switch SQ, the slab of kneighbors.hip): the clamped squared value is stored in place of its
// square root, with ordinary stores -- the selection kernel reads the slab back at once, while it is still in cache.
// A slab has few rows (64 MiB of it at M = 1024 are 8192 rows: 64 workgroups of BI rows on 256 CUs), so the squared
// form also splits the prototypes over blockIdx.y, sq_share(M, gridDim.y) of them (a multiple of BJ) per workgroup:
// a workgroup shifts W, ww and out to its first prototype and runs the unchanged loop on its share.  A pair's chain does not depend on the
// workgroup that runs it.
//
// Rows with missing entries and metric="manhattan" have their matrices in masked.hip and manhattan.hip
// (direct_dist_kernel, direct_rows.h).
#include <math.h>

#include <algorithm>

#include "bmu_common.h"
#include "bmu_tiles.h"

namespace dbgsom {

typedef double d2_t __attribute__((ext_vector_type(2)));
constexpr int64_t SQ_FILL_BLOCKS = 512;   // squared form: the grid launch_distances_form aims at (2 x 256 CUs)
// squared form: prototypes per workgroup when `shares` workgroups divide M among them, in whole chunks of BJ
__host__ __device__ __forceinline__ int sq_share(int M, int shares) {
    return ((M + BJ - 1) / BJ + shares - 1) / shares * BJ;
}

__device__ __forceinline__ void swap_halves(uint32_t &a, uint32_t &b) {   // a's lanes 32..63 <-> b's lanes 0..31
    const auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
    a = r[0]; b = r[1];
}
__device__ __forceinline__ void swap_rows(uint32_t &a, uint32_t &b) {     // a's odd rows of 16 lanes <-> b's even rows
    const auto r = __builtin_amdgcn_permlane16_swap(a, b, false, false);
    a = r[0]; b = r[1];
}

// v[r] of lane (lr, lq) -> v[lq] of lane (lr, r): the transposition of the 4 x 4 block the lanes l, l + 16, l + 32,
// l + 48 hold (every lane of the wavefront takes part)
__device__ __forceinline__ void exchange4(double (&v)[4]) {
    uint32_t lo[4], hi[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { lo[r] = (uint32_t)__double2loint(v[r]); hi[r] = (uint32_t)__double2hiint(v[r]); }
    swap_halves(lo[0], lo[2]); swap_halves(hi[0], hi[2]);
    swap_halves(lo[1], lo[3]); swap_halves(hi[1], hi[3]);
    swap_rows(lo[0], lo[1]); swap_rows(hi[0], hi[1]);
    swap_rows(lo[2], lo[3]); swap_rows(hi[2], hi[3]);
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = __hiloint2double((int)hi[r], (int)lo[r]);
}

// One 16 x 16 tile of a wavefront: a[r] = <x_i, w_j> of row i against prototype jt0 + 4 r + lq (y[r] its norm).
// ovec (wave-uniform): after the exchange this lane stores prototypes jt0 + 4 lq .. + 3 of row i, 16 bytes at a
// time; otherwise the values go out where they are, 8 bytes each -- the four lanes of a row then write 32
// contiguous bytes per instruction, and the exchange would buy nothing.
template <bool SQ, typename T>
__device__ __forceinline__ void put(T v, T *p) {
    if constexpr (SQ) *p = v;
    else __builtin_nontemporal_store(v, p);
}

template <bool SQ, Metric ME>
__device__ __forceinline__ void store_tile(const d4_t &a, double xi, const double (&y)[4], double *__restrict__ out,
                                           int64_t i, int64_t N, int64_t ldo, int jt0, int lq, int M, int ovec) {
    double v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if constexpr (ME == Metric::COSINE) {   // xi = u_i, y = v_j: the value of the cosine search, no root
            v[r] = pair_value_cosine(a[r], xi, y[r]);
        } else {
            double rv = (xi + (-2.0 * a[r])) + y[r];
            if (!(rv > 0.0)) rv = (rv != rv) ? rv : 0.0;  // max(r, 0), NaN kept
            v[r] = SQ ? rv : sqrt(rv);
        }
    }
    if (ovec) {
        exchange4(v);
        const int j0 = jt0 + 4 * lq;
        if (i < N && j0 < M) {
            double *p = out + i * ldo + j0;
            if (j0 + 4 <= M) {
                put<SQ>(d2_t{v[0], v[1]}, reinterpret_cast<d2_t *>(p));
                put<SQ>(d2_t{v[2], v[3]}, reinterpret_cast<d2_t *>(p + 2));
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (j0 + c < M) put<SQ>(v[c], p + c);
            }
        }
    } else if (i < N) {
        double *p = out + i * ldo + jt0 + lq;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (jt0 + 4 * r + lq < M) put<SQ>(v[r], p + 4 * r);
    }
}

// ---------------------------------------------------------------------------------------------
// register-staged form: the product loop of bmu_kernel
// ---------------------------------------------------------------------------------------------
template <typename XT, bool SQ, Metric ME = Metric::L2>
__global__ __launch_bounds__(NT, 2) void dist_kernel(
    const XT *__restrict__ X, int64_t N, int d, int64_t ldx, const double *__restrict__ xx,
    const double *__restrict__ W, int M, const double *__restrict__ ww, int xvec, int wvec,
    double *__restrict__ out, int64_t ldo, int ovec) {
    if constexpr (SQ) {   // this workgroup's share of the prototypes (launch_distances_form: no share is empty)
        const int jsplit = sq_share(M, gridDim.y), j0 = blockIdx.y * jsplit;
        W += (int64_t)j0 * d; ww += j0; out += j0;
        M = min(M - j0, jsplit);
    }
    __shared__ __attribute__((aligned(16))) double xs[2][BI * LS];
    __shared__ __attribute__((aligned(16))) double wsm[2][BJ * LS];
    __shared__ double yy_s[2][BJ];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1;  // 2 x 2 wavefronts: sample half, prototype half
    const int lr = lane & 15, lq = lane >> 4;
    const int64_t i0 = (int64_t)blockIdx.x * BI;

    double xi[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int64_t i = i0 + wi * 64 + it * 16 + lr;
        xi[it] = (i < N) ? xx[i] : 0.0;
    }

    const int lrow = tid >> 1, lk = (tid & 1) * 8;  // staging: 2 threads per tile row, 8 values each
    const int nkt = (d + KT - 1) / KT;
    const int nchunk = (M + BJ - 1) / BJ;
    const int ntile = nkt * nchunk;  // flat (chunk, k-tile) sequence: the pipeline never drains
    XT xr[8];
    double wr[8];

    auto stage_store = [&](int buf) {
        double *xd = &xs[buf][lrow * LS + lk];
        double *wd = &wsm[buf][lrow * LS + lk];
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
            *reinterpret_cast<double2 *>(xd + e) =
                double2{widen(xr[e]), widen(xr[e + 1])};
            *reinterpret_cast<double2 *>(wd + e) = double2{wr[e], wr[e + 1]};
        }
    };

    d4_t acc[4][4];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int it = 0; it < 4; ++it) acc[jt][it] = d4_t{0.0, 0.0, 0.0, 0.0};

    load8<XT>(X, i0 + lrow, N, ldx, lk, d, xvec, xr);
    load8<double>(W, (int64_t)lrow, M, d, lk, d, wvec, wr);
    if (tid < BJ) yy_s[0][tid] = (tid < M) ? ww[tid] : 0.0;
    stage_store(0);
    __syncthreads();

    int kt = 0, jc = 0, parity = 0;
    for (int t = 0; t < ntile; ++t) {
        const int cur = t & 1;
        int kt_n = kt + 1, jc_n = jc;
        if (kt_n == nkt) { kt_n = 0; jc_n = jc + BJ; }
        const bool more = (t + 1 < ntile);
        if (more) {  // the next tile's global loads fly under this tile's MFMAs
            const int kn = kt_n * KT + lk;
            load8<XT>(X, i0 + lrow, N, ldx, kn, d, xvec, xr);
            load8<double>(W, (int64_t)jc_n + lrow, M, d, kn, d, wvec, wr);
            if (kt_n == 0 && tid < BJ)
                yy_s[parity ^ 1][tid] = (jc_n + tid < M) ? ww[jc_n + tid] : 0.0;
        }
#pragma unroll
        for (int ks = 0; ks < KT / 4; ++ks) {
            if (ks == KT / 8 && more) stage_store(cur ^ 1);  // half-way: loads have landed
            double a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                a[u] = wsm[cur][(wj * 64 + u * 16 + lr) * LS + ks * 4 + lq];
                b[u] = xs[cur][(wi * 64 + u * 16 + lr) * LS + ks * 4 + lq];
            }
#pragma unroll
            for (int jt = 0; jt < 4; ++jt)
#pragma unroll
                for (int it = 0; it < 4; ++it)
                    acc[jt][it] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[jt], b[it], acc[jt][it],
                                                                       0, 0, 0);
        }
        if (kt == nkt - 1) {
            // chunk epilogue: every distance of the chunk, exchanged and stored
#pragma unroll
            for (int jt = 0; jt < 4; ++jt) {
                const int jl = wj * 64 + jt * 16;
                double y[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) y[r] = yy_s[parity][jl + 4 * r + lq];
#pragma unroll
                for (int it = 0; it < 4; ++it) {
                    store_tile<SQ, ME>(acc[jt][it], xi[it], y, out, i0 + wi * 64 + it * 16 + lr, N, ldo, jc + jl, lq, M,
                               ovec);
                    acc[jt][it] = d4_t{0.0, 0.0, 0.0, 0.0};
                }
            }
            parity ^= 1;
        }
        __syncthreads();  // tile t+1 is complete in LDS; tile t's buffer may be overwritten next
        kt = kt_n;
        jc = jc_n;
    }
}

// ---------------------------------------------------------------------------------------------
// LDS-DMA form: the product loop of bmu_dma_kernel (3-stage ring, counted vmcnt).  The epilogue's stores count in
// vmcnt as the DMA loads do; loads return in order among themselves, so "all but the youngest tile's worth"
// still means that the older tile has landed -- the wait behind a chunk's epilogue is merely longer than needed.
// ---------------------------------------------------------------------------------------------
template <typename XT, int JTW, bool SQ, Metric ME = Metric::L2>
__global__ __launch_bounds__(NT, 2) void dist_dma_kernel(
    const XT *__restrict__ X, int64_t N, int d, int64_t ldx, const double *__restrict__ xx,
    const double *__restrict__ W, int M, const double *__restrict__ ww, double *__restrict__ out,
    int64_t ldo, int ovec) {
    if constexpr (SQ) {   // this workgroup's share of the prototypes (launch_distances_form: no share is empty)
        const int jsplit = sq_share(M, gridDim.y), j0 = blockIdx.y * jsplit;
        W += (int64_t)j0 * d; ww += j0; out += j0;
        M = min(M - j0, jsplit);
    }
    using XL = XTile<XT>;
    constexpr int BJW = 32 * JTW, W_BYTES = BJW * W_ROW_BYTES, W_DMA_PER_WAVE = JTW;
    constexpr int STAGE_BYTES = XL::BYTES + W_BYTES;
    __shared__ __attribute__((aligned(16))) char smem[NSTAGE * STAGE_BYTES];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wi = wave >> 1, wj = wave & 1;
    const int lr = lane & 15, lq = lane >> 4;
    const int64_t i0 = (int64_t)blockIdx.x * BI;

    double xi[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int64_t i = i0 + wi * 64 + it * 16 + lr;
        xi[it] = (i < N) ? xx[i] : 0.0;
    }

    // ---- per-lane DMA sources (as bmu_dma_kernel) --------------------------------------------
    const XT *xsrc[XL::DMA_PER_WAVE];
#pragma unroll
    for (int u = 0; u < XL::DMA_PER_WAVE; ++u) {
        const int L = 64 * (XL::DMA_PER_WAVE * wave + u) + lane;
        const int r = L / XL::CHUNKS, cp = L % XL::CHUNKS;
        const int c = cp ^ ((r >> 1) & (XL::CHUNKS - 1));
        int64_t row = i0 + r;
        row = row < N ? row : N - 1;  // clamped rows are computed but never stored
        xsrc[u] = X + row * ldx + c * (16 / (int)sizeof(XT));
    }
    int wrow[W_DMA_PER_WAVE], wcol[W_DMA_PER_WAVE];
#pragma unroll
    for (int u = 0; u < W_DMA_PER_WAVE; ++u) {
        const int L = 64 * (W_DMA_PER_WAVE * wave + u) + lane;
        const int r = L / W_CHUNKS, cp = L % W_CHUNKS;
        wrow[u] = r;
        wcol[u] = (cp ^ ((r >> 1) & 7)) * 2;
    }

    const int nkt = d / KT;
    const int nchunk = (M + BJW - 1) / BJW;
    const int ntile = nkt * nchunk;

    auto issue = [&](int t) {  // enqueue the DMA of tile t into ring slot t % NSTAGE
        const int c_t = t / nkt, k0 = (t - c_t * nkt) * KT, jc_t = c_t * BJW;
        char *stage = smem + (t % NSTAGE) * STAGE_BYTES;
#pragma unroll
        for (int u = 0; u < XL::DMA_PER_WAVE; ++u)
            dma16(xsrc[u] + k0, stage + 1024 * (XL::DMA_PER_WAVE * wave + u));
#pragma unroll
        for (int u = 0; u < W_DMA_PER_WAVE; ++u) {
            int j = jc_t + wrow[u];
            j = j < M ? j : M - 1;
            dma16(W + (int64_t)j * d + k0 + wcol[u],
                  stage + XL::BYTES + 1024 * (W_DMA_PER_WAVE * wave + u));
        }
    };
    constexpr int DMA_PER_TILE = XL::DMA_PER_WAVE + W_DMA_PER_WAVE;  // per wave

    // ---- fragment read offsets (bytes inside a stage) ----------------------------------------
    int a_off[JTW], a_swz[JTW], b_off[4], b_swz[4];
#pragma unroll
    for (int u = 0; u < JTW; ++u) {
        const int ra = wj * 16 * JTW + u * 16 + lr;
        a_off[u] = XL::BYTES + ra * W_ROW_BYTES + (lq & 1) * 8;
        a_swz[u] = (ra >> 1) & 7;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int rb = wi * 64 + u * 16 + lr;
        if constexpr (sizeof(XT) == 4) {
            b_off[u] = rb * XL::ROW_BYTES + lq * 4;
            b_swz[u] = (rb >> 1) & 3;
        } else {
            b_off[u] = rb * XL::ROW_BYTES + (lq & 1) * 8;
            b_swz[u] = (rb >> 1) & 7;
        }
    }

    d4_t acc[JTW][4];
#pragma unroll
    for (int jt = 0; jt < JTW; ++jt)
#pragma unroll
        for (int it = 0; it < 4; ++it) acc[jt][it] = d4_t{0.0, 0.0, 0.0, 0.0};

    issue(0);
    if (ntile > 1) issue(1);

    int kt = 0, jc = 0;
    for (int t = 0; t < ntile; ++t) {
        if (t + 1 < ntile) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(DMA_PER_TILE) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (t + 2 < ntile) issue(t + 2);

        const char *stage = smem + (t % NSTAGE) * STAGE_BYTES;
#pragma unroll
        for (int ks = 0; ks < KT / 4; ++ks) {
            double a[JTW], b[4];
#pragma unroll
            for (int u = 0; u < JTW; ++u) {
                const int ca = (2 * ks + (lq >> 1)) ^ a_swz[u];
                a[u] = *reinterpret_cast<const double *>(stage + a_off[u] + ca * 16);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if constexpr (sizeof(XT) == 4) {
                    const int cb = ks ^ b_swz[u];
                    b[u] = (double)*reinterpret_cast<const float *>(stage + b_off[u] + cb * 16);
                } else {
                    const int cb = (2 * ks + (lq >> 1)) ^ b_swz[u];
                    b[u] = *reinterpret_cast<const double *>(stage + b_off[u] + cb * 16);
                }
            }
#pragma unroll
            for (int jt = 0; jt < JTW; ++jt)
#pragma unroll
                for (int it = 0; it < 4; ++it)
                    acc[jt][it] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[jt], b[it], acc[jt][it],
                                                                       0, 0, 0);
        }
        if (kt == nkt - 1) {
            // chunk epilogue (plain loads of |w|^2: once per chunk, L2 resident)
#pragma unroll
            for (int jt = 0; jt < JTW; ++jt) {
                const int jb = jc + wj * 16 * JTW + jt * 16;
                double y[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = jb + 4 * r + lq;
                    y[r] = (j < M) ? ww[j] : 0.0;
                }
#pragma unroll
                for (int it = 0; it < 4; ++it) {
                    store_tile<SQ, ME>(acc[jt][it], xi[it], y, out, i0 + wi * 64 + it * 16 + lr, N, ldo, jb, lq, M, ovec);
                    acc[jt][it] = d4_t{0.0, 0.0, 0.0, 0.0};
                }
            }
            kt = 0;
            jc += BJW;
        } else {
            ++kt;
        }
    }
}

// ---------------------------------------------------------------------------------------------
static int distances_check(int x_dtype, int64_t N, int64_t d, int64_t ldx, int64_t M, int64_t ldo) {
    DBGSOM_REQUIRE(valid_dtype(x_dtype), "x_dtype must be DBGSOM_F32/F64/BF16");
    DBGSOM_REQUIRE(N >= 0 && d >= 1 && ldx >= d && d <= 0x7fffffff, "bad sample shape");
    DBGSOM_REQUIRE(M >= 1 && M <= DBGSOM_MAX_PROTOTYPES, "need 1 <= M <= DBGSOM_MAX_PROTOTYPES");
    DBGSOM_REQUIRE(ldo >= M, "ldo must be >= M");
    return DBGSOM_OK;
}

// SQ: the slab form (ordinary stores, the prototypes split over blockIdx.y; under L2 the squared value).  ME =
// Metric::COSINE: xx holds u, ww holds v (cosine.hip), F32 / F64 rows only; full-matrix and slab form store the same value
template <bool SQ, Metric ME = Metric::L2>
static int launch_distances_form(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx,
                                 const double *W, int64_t M, const double *ww, double *out, int64_t ldo, hipStream_t s) {
    TRY_STATUS(distances_check(x_dtype, N, d, ldx, M, ldo));
    if (ME == Metric::COSINE) DBGSOM_REQUIRE(x_dtype != DBGSOM_BF16, "the cosine matrix takes DBGSOM_F32 or DBGSOM_F64 rows");
    if (N == 0) return DBGSOM_OK;
    DBGSOM_REQUIRE(X && xx && W && ww && out, "null pointer");
    DBGSOM_REQUIRE(is_aligned(out, 8), "out_dev must be 8-byte aligned");
    const int64_t nb = (N + BI - 1) / BI;
    DBGSOM_REQUIRE(nb <= 0x7fffffff, "too many samples for one launch");
    // 16-byte stores: every row base and every group of four prototypes on a 16-byte boundary
    const int ovec = is_aligned(out, 16) && (ldo % 2 == 0);
    // squared form: as many shares of the prototypes (multiples of BJ) as bring the grid to two workgroups per CU
    int shares = 1;
    if (SQ && nb < SQ_FILL_BLOCKS) {
        const int nch = (int)((M + BJ - 1) / BJ);
        shares = (int)std::min<int64_t>((SQ_FILL_BLOCKS + nb - 1) / nb, nch);
        shares = (nch + sq_share((int)M, shares) / BJ - 1) / (sq_share((int)M, shares) / BJ);   // none of them empty
    }
    const int64_t Mb = SQ ? std::min<int64_t>(M, sq_share((int)M, shares)) : M;   // prototypes per workgroup
    dim3 grid((unsigned)nb, (unsigned)shares), block(NT);
    if (bmu_dma_usable(X, x_dtype, d, ldx, W, Mb)) {
        // (dma_chunk_tiles' cost ratios were measured for the search; this epilogue has not been measured apart)
        const int jtw = dma_chunk_tiles(x_dtype, Mb);
#define DBGSOM_DIST_DMA(XT, JTW)                                                                          \
    hipLaunchKernelGGL((dist_dma_kernel<XT, JTW, SQ, ME>), grid, block, 0, s, (const XT *)X, N, (int)d, ldx, xx, W, \
                       (int)M, ww, out, ldo, ovec)
        if (x_dtype == DBGSOM_F32) {
            if (jtw == 1) DBGSOM_DIST_DMA(float, 1);
            else if (jtw == 2) DBGSOM_DIST_DMA(float, 2);
            else DBGSOM_DIST_DMA(float, 4);
        } else {
            if (jtw == 1) DBGSOM_DIST_DMA(double, 1);
            else DBGSOM_DIST_DMA(double, 2);
        }
#undef DBGSOM_DIST_DMA
        return launch_status("dist_dma_kernel");
    }
    const size_t xe = dtype_size(x_dtype);
    const int xvec = is_aligned(X, 16) && ((ldx * xe) % 16 == 0);
    const int wvec = is_aligned(W, 16) && ((d * 8) % 16 == 0);
#define DBGSOM_DIST(XT)                                                                                      \
    hipLaunchKernelGGL((dist_kernel<XT, SQ, ME>), grid, block, 0, s, (const XT *)X, N, (int)d, ldx, xx, W, (int)M, ww, \
                       xvec, wvec, out, ldo, ovec)
    if (x_dtype == DBGSOM_F32) DBGSOM_DIST(float);
    else if (x_dtype == DBGSOM_F64) DBGSOM_DIST(double);
    else if constexpr (ME == Metric::L2) DBGSOM_DIST(bf16_t);
#undef DBGSOM_DIST
    return launch_status("dist_kernel");
}

int launch_distances(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx, const double *W,
                     int64_t M, const double *ww, double *out, int64_t ldo, hipStream_t s) {
    return launch_distances_form<false>(X, x_dtype, N, d, ldx, xx, W, M, ww, out, ldo, s);
}

int launch_distances_squared(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx,
                             const double *W, int64_t M, const double *ww, double *out, int64_t ldo, hipStream_t s) {
    return launch_distances_form<true>(X, x_dtype, N, d, ldx, xx, W, M, ww, out, ldo, s);
}

int launch_distances_cosine(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *u, const double *W,
                            int64_t M, const double *v, double *out, int64_t ldo, hipStream_t s) {
    return launch_distances_form<false, Metric::COSINE>(X, x_dtype, N, d, ldx, u, W, M, v, out, ldo, s);
}

int launch_distances_cosine_slab(const void *X, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *u,
                                 const double *W, int64_t M, const double *v, double *out, int64_t ldo, hipStream_t s) {
    return launch_distances_form<true, Metric::COSINE>(X, x_dtype, N, d, ldx, u, W, M, v, out, ldo, s);
}

}  // namespace dbgsom

using namespace dbgsom;

extern "C" {

int dbgsom_distances(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx_dev,
                     const double *W_dev, int64_t M, const double *ww_dev, double *out_dev, int64_t ldo, void *stream) {
    return launch_distances(X_dev, x_dtype, N, d, ldx, xx_dev, W_dev, M, ww_dev, out_dev, ldo, (hipStream_t)stream);
}

}  // extern "C"
