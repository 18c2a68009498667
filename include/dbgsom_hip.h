/*
 * dbgsom_hip.h -- C ABI of the MI355X (gfx950) batch-SOM hot path.
 *
 * Drop-in boundary for the per-epoch hot path of SandroMartens/DBGSOM.  The reference has
 * no FFI seam of its own: the path sits behind four private methods of `BaseSom` and two
 * numba functions (dbgsom/BaseSom.py).  Each entry point below names the reference
 * interface it replaces (file:line under the reference tree).  INTEGRATION.md shows the
 * ctypes binding a reference maintainer would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch / C++ types.
 *   - every function returns 0 on success, a negative DBGSOM_E* code on failure;
 *     dbgsom_last_error() returns the message of the calling thread's last failure.
 *     HIP errors never cross the ABI as exceptions.
 *   - "dev" pointers are device (HBM) addresses, "host" pointers are host addresses.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Device-level
 *     calls only ENQUEUE work on `stream`; the caller synchronises.  Context-level calls
 *     (dbgsom_ctx_*) are blocking.
 *   - workspaces: a `workspace_dev` / `ws` argument is device scratch of at least the bytes the `dbgsom_*_workspace_bytes`
 *     function declared beside its entry returns for the same shape (exactly that many is enough).  Each entry states
 *     its alignment (16 or 256 bytes).  Unless the entry says otherwise -- dbgsom_bmu_filtered and the calls that share
 *     its workspace are the one exception -- the contents on entry are irrelevant: a buffer may go from call to call,
 *     from shape to shape and from entry to entry without being cleared.  Nothing outside [ptr, ptr + bytes) is ever
 *     written.  A short workspace (DBGSOM_ENOMEM; dbgsom_sparse_code: DBGSOM_EINVAL) and a misaligned one
 *     (DBGSOM_EINVAL) are refused before anything is launched.
 *   - matrices are row-major; `ld*` is the row stride in ELEMENTS.
 *   - handles are not thread-safe; calls are blocking from one host thread per context.
 */
#ifndef DBGSOM_HIP_H
#define DBGSOM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DBGSOM_ABI_VERSION 4

/* sample storage types (the reference accepts float64 and float32 input: SomVQ.py:121-124) */
#define DBGSOM_F32 0
#define DBGSOM_F64 1
#define DBGSOM_BF16 2 /* storage-only extension (bfloat16 bits, exact up-cast; arithmetic stays float64) */

/* layout of the Voronoi-centre rows fed to the smoothing step */
#define DBGSOM_CENTRES_COMPACT 0 /* reference behaviour: BaseSom.py:1045,1053 (row = rank among non-empty neurons) */
#define DBGSOM_CENTRES_ALIGNED 1 /* row = neuron id (the mathematically intended form) */

#define DBGSOM_OK 0
#define DBGSOM_EINVAL (-1)   /* bad argument (shape, dtype, null pointer, k, alignment) */
#define DBGSOM_EHIP (-2)     /* a HIP runtime call failed; see dbgsom_last_error() */
#define DBGSOM_ENOMEM (-3)   /* workspace too small / allocation failed */
#define DBGSOM_ESTATE (-4)   /* context used out of order (e.g. epoch before load) */
#define DBGSOM_ERANGE (-5)   /* a winner index outside [0, M) was met */
#define DBGSOM_ECALLBACK (-6) /* the caller's all-reduce callback reported a failure */

/* OR-ed into `seed_stride` of dbgsom_bmu_filtered: the stateless seed pre-pass looks at every
 * prototype and every feature (as expensive as the candidate sweep it seeds; pays on weakly
 * clustered data, where cheap seeds leave nearly every prototype a candidate) */
#define DBGSOM_SEED_FULL 0x100
/* OR-ed into `seed_stride` as well.  DBGSOM_PRUNE: no candidate sweep -- the candidates of a sample are
 * the prototypes the triangle inequality cannot rule out from the distance to its seed and a certified
 * lower bound of the distances between prototypes (filter.hip section 2c; M <= 8192, otherwise ignored).
 * Same results, by construction; pays on clustered data, where it leaves the sample's own cluster.
 * DBGSOM_PRUNE_PROBE: the sweep as usual, plus a counting-only run of that rule whose list-length sum
 * dbgsom_ctx_epoch_info / the engine's policy reads (what DBGSOM_PRUNE would cost, without paying it). */
#define DBGSOM_PRUNE 0x200
#define DBGSOM_PRUNE_PROBE 0x400
/* with either of the two, in a stateless search with the cheap seed pre-pass: 128-sample workgroups
 * whose pruned lists come out longer than max(96, M / 8) -- their seeds were poor -- are seeded again
 * against every prototype and pruned again (two more short launches) */
#define DBGSOM_PRUNE_RETRY 0x800
/* with DBGSOM_PRUNE on a stateless k = 1 call that brings anchor buckets and their run table
 * (dbgsom_bmu_filtered_anchor_runs), without DBGSOM_PRUNE_RETRY and without DBGSOM_REFINE: the lean form.  The lists
 * written from the anchors' bounds are final, long ones included (each is a valid candidate set: same winners, same
 * distances, only longer lists for those workgroups, which dbgsom_bmu_filtered_anchor_bounds still counts as handed
 * over), and the call makes nothing that only the per-sample pass reads: no digit planes of W, no gap table, no
 * per-sample seeds (dbgsom_bmu_filtered_gaps and the seed_host of dbgsom_bmu_filtered_anchor_seeds are then not
 * those of this call).  Ignored on every other call. */
#define DBGSOM_ANCHOR_LISTS_ONLY 0x2000
/* per-SAMPLE refinement in front of the exact stage: the four int8 digit products of the top two digit
 * planes over each workgroup's candidate list leave every sample the few prototypes a certified bound
 * cannot separate (<= 4, else its whole list); the samples are bucketed again by their likely winner and
 * the float64 chain runs on those (sample, prototype) pairs alone, on the vector ALU, with the gathered
 * rows streamed once.  Workgroups whose lists do not fit the refinement's tile (256 entries) go through
 * the matrix-core stage as without the flag. */
#define DBGSOM_REFINE 0x1000

/* prototype-count limit of the accumulate step (per-block LDS histogram) */
#define DBGSOM_MAX_PROTOTYPES 16000
/* most neighbours per row of the dbgsom_kneighbors* calls (the selection keeps them in registers) */
#define DBGSOM_MAX_NEIGHBORS 32

int dbgsom_abi_version(void);
const char *dbgsom_last_error(void);
/* number of visible HIP devices (0 and DBGSOM_OK when none: the caller decides to fail) */
int dbgsom_device_count(int *count);

/* ------------------------------------------------------------------------------------------
 * Device-level entry points (raw HBM pointers + stream).  One call = one step of the path.
 * ------------------------------------------------------------------------------------------ */

/* out[r] = sum_k A[r,k]^2 in float64, sequential fma chain over k.
 * Replaces the row-norm pre-pass of sklearn's brute engines that BaseSom.py:455-457 calls
 * (`row_norms(..., squared=True)`).  Run once per resident X, once per epoch for W. */
int dbgsom_row_sqnorms(const void *A_dev, int dtype, int64_t rows, int64_t d, int64_t ld,
                       double *out_dev, void *stream);

/* Best-matching-unit search: BaseSom._get_winning_neurons(data, n_bmu)  BaseSom.py:446-464.
 *   r_ij = (|x_i|^2 + (-2 <x_i,w_j>)) + |w_j|^2 in float64, clamp at 0, arg-k-min over j with
 *   ties to the lowest j, dist = sqrt(r).  k in {1,2}.
 *   X: N x d (x_dtype), xx: N squared norms; W: M x d float64 contiguous, ww: M squared norms.
 *   idx: N x k int64, dist: N x k float64 (ascending by (r, j)).
 *   round_f32 != 0 rounds the returned distances through float32 (what the reference's engine
 *   does when samples AND prototypes are float32, i.e. epoch 0 of a float32 fit). */
int dbgsom_bmu(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx,
               const double *xx_dev, const double *W_dev, int64_t M, const double *ww_dev, int k,
               int round_f32, int64_t *idx_dev, double *dist_dev, void *stream);

/* Sample kernel: BaseSom._calculate_exp_similarity(distances)  BaseSom.py:533-538.
 *   kw_i = 1 - sqrt(1 - exp(-gamma * dist_i^2)),  gamma = 1 / total_variance. */
int dbgsom_exp_similarity(const double *dist_dev, int64_t N, double gamma, double *kw_dev,
                          void *stream);

/* Per-neuron sums of one epoch, id-indexed, deterministic (stable counting sort by winner +
 * ordered segmented reduction; no floating-point atomics):
 *   S_j = sum_{i: win_i=j} kw_i x_i   numba_voronoi_set_centers numerator  BaseSom.py:1028-1055
 *   K_j = sum kw_i                     its denominator
 *   a_j = |{i}|                        neuron_activations                   BaseSom.py:500-503
 *   E_j = sum dist_i                   numba_quantization_error             BaseSom.py:1058-1073
 * sums_dev holds M*(d+3) float64:  [ S (M*d) | K (M) | a (M) | E (M) ]  -- the buffer a
 * sample-sharded multi-GPU run all-reduces (one collective per epoch).
 * status_dev (int32[1], may be NULL) is set non-zero when a winner is outside [0,M) (that
 * sample is skipped).
 * Workspace: 256-byte aligned, contents on entry irrelevant, nothing outside [workspace_dev, workspace_dev +
 * workspace_bytes) is written. */
size_t dbgsom_accumulate_workspace_bytes(int64_t N, int64_t d, int64_t M);
int dbgsom_accumulate(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx,
                      const int64_t *idx_dev, const double *kw_dev, const double *dist_dev,
                      int64_t M, double *sums_dev, int32_t *status_dev, void *workspace_dev,
                      size_t workspace_bytes, void *stream);

/* The same sums with a weight per row (sw_dev: N float64, finite and >= 0 -- not checked here): a row of
 * weight w counts as w copies of that row,
 *   S_j = sum sw_i kw_i x_i,  K_j = sum sw_i kw_i,  a_j = sum sw_i,  E_j = sum sw_i dist_i.
 * a_j is an ordered float64 sum like K_j and E_j (list order, chunk order, group order: bitwise
 * reproducible, independent of the grid); rows of weight 0 are not streamed and contribute to nothing.
 * The first N int32 of the workspace hold the sample ids bucketed by winner as after dbgsom_accumulate
 * (rows of weight 0 included: the sort does not look at weights, the sums skip those rows).
 * Workspace: 256-byte aligned, contents on entry irrelevant, nothing outside [workspace_dev, workspace_dev +
 * workspace_bytes) is written. */
size_t dbgsom_accumulate_weighted_workspace_bytes(int64_t N, int64_t d, int64_t M);
int dbgsom_accumulate_weighted(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx,
                               const int64_t *idx_dev, const double *kw_dev, const double *sw_dev,
                               const double *dist_dev, int64_t M, double *sums_dev, int32_t *status_dev,
                               void *workspace_dev, size_t workspace_bytes, void *stream);

/* ---- CSR samples (csr.hip) ----------------------------------------------------------------------------
 * Canonical CSR: indptr int64 (N + 1, indptr[0] = 0, indptr[N] = nnz, monotone), indices int32 in [0, d),
 * strictly ascending within a row (no duplicates), data float32 or float64; explicitly stored zeros are allowed.
 * Every kernel walks the stored entries of a row in ascending column order with the arithmetic of its dense
 * namesake, so its results are the dense kernel's on the densified matrix BIT FOR BIT: a term x_k = 0 leaves a
 * chain acc = fma(x_k, w_k, acc) and an ordered sum where they were.
 *
 * dbgsom_csr_check: host arrays, needs no GPU; DBGSOM_EINVAL and a message naming the first fault.
 * dbgsom_csr_row_sqnorms: xx_i, the chain of dbgsom_row_sqnorms over the stored entries.
 * dbgsom_csr_transpose_weights: Wt (d x ldwt float64, ldwt = dbgsom_csr_wt_ld(M), zeros behind column M) from
 *   W (M x ldw): the layout the search reads -- one stored entry, one contiguous run of prototypes.
 * dbgsom_bmu_csr: dbgsom_bmu for CSR samples; ww_dev from dbgsom_row_sqnorms on W.
 * dbgsom_csr_densify: the padded dense rows (N x ld, X's own dtype).
 * dbgsom_accumulate_csr: dbgsom_accumulate (sw_dev = NULL) / dbgsom_accumulate_weighted for CSR samples; sums_dev
 *   holds M*(d+3) float64 with the d given here, any d >= 1 (the context passes its padded feature count); the
 *   status word, the skipped rows and the first N int32 of the workspace are the dense calls'; the workspace size
 *   is that of the weighted call for both forms.  Bit-identical to the dense call wherever that one adds a column
 *   in list order, which is from 256 pieces per row on: 16-byte pieces when X_dev and ldx are 16-byte aligned and
 *   d is a multiple of the piece (d >= 1024 for float32, >= 512 for float64, as with the context's padded rows),
 *   single elements otherwise (any d >= 256); narrower dense rows are summed over row lanes, in another order.
 *   Workspace: 256-byte aligned, contents on entry irrelevant, nothing outside [workspace_dev, workspace_dev +
 * workspace_bytes) is written. */
int dbgsom_csr_check(const int64_t *indptr_host, const int32_t *indices_host, int64_t N, int64_t d, int64_t nnz);
int dbgsom_csr_row_sqnorms(const int64_t *indptr_dev, const void *data_dev, int x_dtype, int64_t N, double *out_dev,
                           void *stream);
int64_t dbgsom_csr_wt_ld(int64_t M);
int dbgsom_csr_transpose_weights(const double *W_dev, int64_t M, int64_t d, int64_t ldw, double *Wt_dev, int64_t ldwt,
                                 void *stream);
int dbgsom_bmu_csr(const int64_t *indptr_dev, const int32_t *indices_dev, const void *data_dev, int x_dtype, int64_t N,
                   const double *xx_dev, const double *Wt_dev, int64_t ldwt, int64_t M, const double *ww_dev, int k,
                   int round_f32, int64_t *idx_dev, double *dist_dev, void *stream);
int dbgsom_csr_densify(const int64_t *indptr_dev, const int32_t *indices_dev, const void *data_dev, int x_dtype,
                       int64_t N, int64_t d, int64_t ld, void *out_dev, void *stream);
size_t dbgsom_accumulate_csr_workspace_bytes(int64_t N, int64_t d, int64_t M);
int dbgsom_accumulate_csr(const int64_t *indptr_dev, const int32_t *indices_dev, const void *data_dev, int x_dtype,
                          int64_t N, int64_t d, const int64_t *idx_dev, const double *kw_dev, const double *sw_dev,
                          const double *dist_dev, int64_t M, double *sums_dev, int32_t *status_dev,
                          void *workspace_dev, size_t workspace_bytes, void *stream);

/* Neighbourhood-weighted batch update: steps 3-5 of BaseSom._update_weights
 * BaseSom.py:506-522 with _calculate_gaussian_neighborhood BaseSom.py:525-531.
 *   c_j = S_j / K_j placed per `layout`;  h = exp(-(hop^2 / (2 sigma^2)));
 *   W'_i = sum_j h_ij a_j c_j / sum_j h_ij a_j;   change_total = sum_i |W_i - W'_i|_2.
 * hop: M x M float32 lattice hop counts (+inf when disconnected).  W_new may not alias W_old.
 * change_total_dev: one float64 on the device.
 * Workspace: 256-byte aligned, contents on entry irrelevant, nothing outside [workspace_dev, workspace_dev +
 * workspace_bytes) is written. */
size_t dbgsom_smooth_workspace_bytes(int64_t M, int64_t d);
int dbgsom_smooth(const double *sums_dev, int64_t M, int64_t d, const float *hop_dev,
                  double sigma, int layout, const double *W_old_dev, double *W_new_dev,
                  double *change_total_dev, void *workspace_dev, size_t workspace_bytes,
                  void *stream);

/* ---- filtered BMU search: identical results, most float64 work removed -------------------------
 * An int8-MFMA sweep over 3 x 8-bit digit planes of X and W bounds every r_ij with a rigorous
 * per-sample error eps_i; prototype j stays a candidate of a 128-sample workgroup when
 * r~_ij <= r~_{i,prev(i)} + 2 eps_i for one of its samples (prev = winner of the previous epoch);
 * the exact float64 search (same arithmetic as dbgsom_bmu) then runs on the candidates only.
 * Same reference step as dbgsom_bmu (BaseSom.py:446-464), k = 1, float32 or float64 samples,
 * d % 16 == 0 (callers pad rows with zeros: zeros change no fma chain).
 *   xplanes_dev : filled once per fit by dbgsom_filter_prepare (digit planes + row scales of X)
 *   prev_idx_dev: N winners of the previous epoch (any valid indices < M keep the result exact;
 *                 good ones keep the candidate sets small)
 *   order_dev   : the N sample ids bucketed by prev_idx -- the first N int32 of the workspace of
 *                 the previous dbgsom_accumulate call
 *   prev_idx_dev = order_dev = NULL: stateless form -- a coarser int8 pre-pass (three digit
 *                 products, every seed_stride-th prototype; 0 = default: ceil(M / 256), at least 4; on the three 64-feature
 *                 blocks in which the prototypes differ most) finds a starting
 *                 prototype per sample and the samples are bucketed by it; nothing from an earlier
 *                 call is used.  The seed only sets the candidate threshold: ANY seed gives the
 *                 exact result, a nearer one shorter candidate lists.  DBGSOM_SEED_FULL, DBGSOM_PRUNE,
 *                 DBGSOM_PRUNE_PROBE and DBGSOM_PRUNE_RETRY (above) are OR-ed into this argument.
 *   sweep_planes: digit planes per operand in the candidate sweep: 3 = six digit products (error
 *                 bound ~1e-6 of |x||w|), 2 = three products (bound ~3e-4, half the MFMA work and
 *                 two thirds of the traffic, somewhat longer candidate lists), 1 = one product
 *                 (bound ~5e-2, half the time of 2 again; enough where the candidates are the
 *                 sample's cluster anyway); 0 = default (2).  Results never depend on it. */
size_t dbgsom_filter_planes_bytes(int64_t rows, int64_t d);
int dbgsom_filter_prepare(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx,
                          void *planes_dev, size_t planes_bytes, void *stream);
/* The workspace of dbgsom_bmu_filtered must be zero-filled ONCE after it is allocated (its first 256
 * bytes hold self-resetting "last workgroup" tickets); calls leave it ready for the next call.  This is the one
 * workspace whose contents on entry matter; dbgsom_bmu_filtered_anchored and dbgsom_bmu_filtered_anchor_runs share
 * it.  256-byte aligned; nothing outside [workspace_dev, workspace_dev + workspace_bytes) is written. */
size_t dbgsom_bmu_filtered_workspace_bytes(int64_t N, int64_t d, int64_t M);
int dbgsom_bmu_filtered(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx,
                        const double *xx_dev, const void *xplanes_dev, const double *W_dev,
                        int64_t M, const double *ww_dev, const int64_t *prev_idx_dev,
                        const int32_t *order_dev, int seed_stride, int sweep_planes,
                        int round_f32, int64_t *idx_dev, double *dist_dev, void *workspace_dev,
                        size_t workspace_bytes, void *stream);
/* diagnostics: per-stage HIP-event timing of dbgsom_bmu_filtered on the caller's stream.
 * ms5 = [slice W + tables, coarse pre-pass, bucket sort, int8 sweep, exact search on candidates] */
int dbgsom_filter_timing(int enable);
int dbgsom_bmu_filtered_stage_ms(double *ms5);
/* diagnostics: candidate-list length of every 128-sample workgroup of the last filtered call.  Synchronises the
 * stream. */
int dbgsom_bmu_filtered_counts(const void *workspace_dev, int64_t N, int64_t d, int64_t M,
                               uint32_t *counts_host, int64_t n_counts, void *stream);
/* the same copy queued on `stream` without synchronising: counts_host must be page-locked and is
 * valid once the caller has synchronised the stream */
int dbgsom_bmu_filtered_counts_async(const void *workspace_dev, int64_t N, int64_t d, int64_t M,
                                     uint32_t *counts_host, int64_t n_counts, void *stream);
/* diagnostics: the gap table of the triangle-inequality form, gap_host[p * M + j] <= |w_p - w_j|^2 (M x M float32,
 * symmetric bit for bit; 0 = no gap known: the diagonal, duplicates, rows with a NaN or an infinity).  Valid after a call with DBGSOM_PRUNE
 * or DBGSOM_PRUNE_PROBE on this workspace with the same N, d, M; M > 8192 (no table) is DBGSOM_EINVAL.  Synchronises
 * the stream. */
int dbgsom_bmu_filtered_gaps(const void *workspace_dev, int64_t N, int64_t d, int64_t M, float *gap_host,
                             void *stream);
/* The stateless call seeded from anchor buckets the caller built (what the context does once per load, see
 * "anchor_seeds"): no seed pre-pass and no sort.  anchors_dev: n_anchors x d float64, contiguous, 16-byte aligned
 * (rows of the samples, or any points near them), 1 <= n_anchors <= 256; anchor_of_dev[i] in [0, n_anchors): the
 * anchor sample i is grouped with; order_dev: the N sample ids bucketed by anchor_of.  Each anchor's nearest prototype
 * (float64, the lowest index among equals; a row with a NaN, an infinity or an overflowing norm only when no finite
 * row exists) seeds the samples grouped with it.  Only the pruning form: seed_stride carries DBGSOM_PRUNE and not
 * DBGSOM_SEED_FULL, otherwise DBGSOM_EINVAL.  Winners and distances are dbgsom_bmu_filtered's, whatever the buckets. */
int dbgsom_bmu_filtered_anchored(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx,
                                 const double *xx_dev, const void *xplanes_dev, const double *W_dev,
                                 int64_t M, const double *ww_dev, const double *anchors_dev, int n_anchors,
                                 const int32_t *anchor_of_dev, const int32_t *order_dev, int seed_stride,
                                 int sweep_planes, int round_f32, int64_t *idx_dev, double *dist_dev,
                                 void *workspace_dev, size_t workspace_bytes, void *stream);
/* diagnostics: the seeds of the last dbgsom_bmu_filtered_anchored call on this workspace with the same N, d, M:
 * aseed_host[a] the prototype chosen for anchor a (n_anchors int32), seed_host[i] the seed of sample i (N int64; may
 * be NULL; with DBGSOM_PRUNE_RETRY the re-seeding pass has overwritten some).  M > 8192 is DBGSOM_EINVAL.
 * Synchronises the stream. */
int dbgsom_bmu_filtered_anchor_seeds(const void *workspace_dev, int64_t N, int64_t d, int64_t M, int n_anchors,
                                     int32_t *aseed_host, int64_t *seed_host, void *stream);
/* The run table of anchor buckets: for every 128-sample workgroup g of order_dev its runs of equal anchor,
 * [run_start[g], run_start[g + 1]), each as (anchor, R, XXmax): R >= max |x_i - a| over the run's samples (float64 sum of
 * squared differences, widened by the relative margin (d + 8) 2^-52), XXmax = max xx_dev[i].  A run with a row, a norm
 * or an anchor that is not finite has R = XXmax = +inf.  A function of the samples and the buckets alone: build it
 * once, pass it to any number of dbgsom_bmu_filtered_anchor_runs calls.  X_dev: F32 / F64 / BF16 rows, the values the
 * search reads.  runs_dev: dbgsom_anchor_runs_bytes(N, n_anchors) bytes, 256-byte aligned.  The table holds N / 128 +
 * n_anchors runs (rounded up) -- enough for buckets in ascending order of the anchor; a workgroup whose runs did not
 * fit takes the whole map as candidates. */
size_t dbgsom_anchor_runs_bytes(int64_t N, int n_anchors);
int dbgsom_anchor_runs_build(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx_dev,
                             const double *anchors_dev, int n_anchors, const int32_t *anchor_of_dev,
                             const int32_t *order_dev, void *runs_dev, size_t runs_bytes, void *stream);
/* diagnostics: the table on the host.  run_start_host: ceil(N / 128) + 1 int32; the other arrays (each may be NULL):
 * ceil(N / 128) + n_anchors entries at the most, the first min(run_start[last], that) are written.  Synchronises. */
int dbgsom_anchor_runs_read(const void *runs_dev, int64_t N, int n_anchors, int32_t *run_start_host,
                            int32_t *run_anchor_host, double *run_R_host, double *run_xx_host, void *stream);
/* dbgsom_bmu_filtered_anchored with the run table of its buckets (k = 1, stateless, DBGSOM_PRUNE): the candidate lists
 * come from certified bounds of the distances between the anchors and the prototypes and the table -- no pass over the
 * samples' planes; only workgroups whose lists that leaves longer than max(M / 8, 96) get the per-sample pass of
 * dbgsom_bmu_filtered_anchored.  Winners and distances are the same bits. */
int dbgsom_bmu_filtered_anchor_runs(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx,
                                    const double *xx_dev, const void *xplanes_dev, const double *W_dev,
                                    int64_t M, const double *ww_dev, const double *anchors_dev, int n_anchors,
                                    const int32_t *anchor_of_dev, const int32_t *order_dev, const void *runs_dev,
                                    int seed_stride, int sweep_planes, int round_f32, int64_t *idx_dev, double *dist_dev,
                                    void *workspace_dev, size_t workspace_bytes, void *stream);
/* diagnostics: the candidate lists of the last filtered call on this workspace with the same N, d, M: lists_host[g * M
 * + k], k < counts[g] (dbgsom_bmu_filtered_counts), the ascending prototype ids of workgroup g (ceil(N / 128) x M
 * uint16; what lies behind a list's length is not defined).  Synchronises the stream. */
int dbgsom_bmu_filtered_lists(const void *workspace_dev, int64_t N, int64_t d, int64_t M, uint16_t *lists_host,
                              void *stream);
/* diagnostics: the bounds of the last dbgsom_bmu_filtered_anchor_runs call on this workspace with the same N, d, M:
 * low_host[a * M + j] <= |a - w_j|^2 (n_anchors x M float32; 0 = no bound known), up_host[a] >= |a - w_seed(a)|
 * (n_anchors float64; +inf = none), counts2_host = [workgroups handed to the per-sample pass, workgroups whose lists
 * were still long after it].  Every array may be NULL.  Synchronises the stream. */
int dbgsom_bmu_filtered_anchor_bounds(const void *workspace_dev, int64_t N, int64_t d, int64_t M, int n_anchors,
                                      float *low_host, double *up_host, uint64_t *counts2_host, void *stream);

/* diagnostics of the per-sample refinement (DBGSOM_REFINE) of the last filtered call:
 * out4 = [(sample, prototype) pairs evaluated exactly, 128-sample workgroups refined (the others went
 * through the matrix-core stage), samples whose candidates did not fit four slots (evaluated against
 * their workgroup's whole list), distinct candidates summed over the pair kernel's 64-sample workgroups];
 * synchronises the stream */
int dbgsom_bmu_filtered_refine_counts(const void *workspace_dev, int64_t N, int64_t d, int64_t M,
                                      uint64_t *out4, void *stream);

/* ---- post-fit consumers of the BMU step as device reductions (N-sized arrays stay in HBM) ---- */

/* out[0] = sum of v[0..n) with a fixed reduction tree (bitwise reproducible).  Mean BMU distance =
 * BaseSom.calculate_quantization_error  BaseSom.py:904-922.
 * Workspace: 16-byte aligned, contents on entry irrelevant, nothing outside [workspace_dev, workspace_dev +
 * workspace_bytes) is written. */
size_t dbgsom_sum_workspace_bytes(void);
int dbgsom_sum_f64(const double *v_dev, int64_t n, double *out_dev, void *workspace_dev,
                   size_t workspace_bytes, void *stream);

/* count of samples whose two BMUs (idx2: n x 2 from dbgsom_bmu with k=2) are further than 1.5
 * apart on the lattice; xy: M x 2 int32 neuron coordinates.
 * BaseSom._calculate_topographic_error  BaseSom.py:924-953 (its Python loop over the samples). */
int dbgsom_topographic_count(const int64_t *idx2_dev, int64_t n, const int32_t *xy_dev, int64_t M,
                             uint64_t *count_dev, void *stream);

/* out[j] = sum_i X[i, j] (mean == NULL) or sum_i (X[i, j] - mean[j])^2, each column summed
 * sequentially over the rows in X's own dtype without fused multiply-add: the arithmetic of
 * NumPy's axis-0 reductions, so that np.var / np.std of the resident samples -- the total
 * variance behind the sample kernel (BaseSom.py:363) and the "se" growing threshold
 * (BaseSom.py:380-383) -- come out bit for bit without a host pass over X.  F32 / F64 only;
 * out, mean: d elements of X's dtype on the device. */
int dbgsom_column_sums(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx,
                       const void *mean_dev, void *out_dev, void *stream);

/* out_i = exp(-dist_i^2 / (2 sigma^2)) / (sigma sqrt(2 pi)): the per-sample term of the local
 * density estimate, BaseSom._calculate_node_statistics BaseSom.py:203-206.  Feeding it to
 * dbgsom_accumulate as `kw` yields per-neuron density sums (K) and hit counts (a). */
int dbgsom_density_terms(const double *dist_dev, int64_t n, double sigma, double *out_dev,
                         void *stream);

/* Weighted forms of the reductions above (w_dev: one float64 weight per row).  Floating-point sums without
 * atomics: fixed grids and ordered partials, bitwise reproducible.
 *   dbgsom_weighted_sum_f64   out = sum_i w_i v_i (v_dev == NULL: sum_i w_i); workspace as dbgsom_sum_f64
 *   dbgsom_topographic_weight out = summed weight of the rows dbgsom_topographic_count counts
 *   dbgsom_class_histogram_weighted  hist[j, c] = summed weight of the rows of class c in neuron j's list:
 *       order_dev = the N sample ids bucketed by winner (stable), seg_start_dev = the M + 1 exclusive list starts
 *       (seg_start[M] = N); added in list order
 *   dbgsom_weighted_column_sums  out[j] = sum_i w_i x_ij (mean_dev == NULL) or sum_i w_i (x_ij - mean_j)^2, in
 *       float64 whatever the storage dtype (mean_dev, out_dev: d float64)
 * Workspaces (dbgsom_sum_workspace_bytes for the two sums, dbgsom_weighted_column_sums_workspace_bytes): 16-byte
 * aligned, contents on entry irrelevant, nothing outside [workspace_dev, workspace_dev + workspace_bytes) is written. */
int dbgsom_weighted_sum_f64(const double *v_dev, const double *w_dev, int64_t n, double *out_dev,
                            void *workspace_dev, size_t workspace_bytes, void *stream);
int dbgsom_topographic_weight(const int64_t *idx2_dev, const double *w_dev, int64_t n, const int32_t *xy_dev,
                              int64_t M, double *out_dev, void *workspace_dev, size_t workspace_bytes,
                              void *stream);
int dbgsom_class_histogram_weighted(const int32_t *order_dev, const uint32_t *seg_start_dev, const int32_t *y_dev,
                                    const double *w_dev, int64_t n, int64_t M, int64_t n_classes,
                                    double *hist_dev, void *stream);
size_t dbgsom_weighted_column_sums_workspace_bytes(int64_t d);
int dbgsom_weighted_column_sums(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx,
                                const double *w_dev, const double *mean_dev, double *out_dev,
                                void *workspace_dev, size_t workspace_bytes, void *stream);

/* hist[j, c] = |{i : win_i = j, y_i = c}| (M x n_classes uint64, integer atomics: exact).
 * Entropy growth criterion BaseSom.py:547-551 and SomClassifier._label_prototypes
 * SomClassifier.py:130-152 (their O(N*M) boolean masks). */
int dbgsom_class_histogram(const int64_t *idx_dev, const int32_t *y_dev, int64_t n, int64_t M,
                           int64_t n_classes, uint64_t *hist_dev, void *stream);

/* ------------------------------------------------------------------------------------------
 * Context-level entry points (host pointers; the library owns the device memory).
 * This is the seam a NumPy caller such as the reference binds with ctypes, and it is THE PRODUCT:
 * the estimators of dbgsom_amd are thin callers of it.  X is uploaded once and stays resident in
 * HBM across epochs; every result is written into caller-allocated, C-contiguous host arrays; no
 * host pointer is retained after a call returns.  Behind it, invisible to the caller: zero-padding
 * of the rows to a multiple of 16 features (changes no fma chain), bfloat16 storage, the cached
 * int8 digit planes, the choice between the all-pairs and the filtered search (always the same
 * results), previous winners as seeds, device-resident prototypes between epochs.
 * All calls are blocking; one host thread per context.
 * ------------------------------------------------------------------------------------------ */
typedef struct dbgsom_ctx dbgsom_ctx;

/* BMU search of a context -- every choice gives IDENTICAL results (option "algorithm") */
#define DBGSOM_ALG_AUTO 0          /* FILTERED_HINT + back-off to EXACT while the candidate lists are long */
#define DBGSOM_ALG_EXACT 1         /* all-pairs float64 MFMA search */
#define DBGSOM_ALG_FILTERED 2      /* stateless: int8 seed pre-pass -> int8 candidate sweep -> exact float64 on candidates */
#define DBGSOM_ALG_FILTERED_HINT 3 /* the same with the previous epoch's winners as seeds when there are any */

/* flags of dbgsom_ctx_epoch */
#define DBGSOM_EPOCH_FROZEN 1 /* the resident prototypes stay what they are (bench: same map every step) */

int dbgsom_ctx_create(int device, dbgsom_ctx **out);
int dbgsom_ctx_destroy(dbgsom_ctx *ctx);

/* Integer options by name.  Settable: "algorithm" (DBGSOM_ALG_*), "sweep_planes" (0 adaptive,
 * 1..3 fixed digit planes of the candidate sweep, 4 = no sweep: candidates from the triangle
 * inequality, DBGSOM_PRUNE), "seed_stride" (0 = library default),
 * "timing" (1: HIP events around the phases of an epoch and the stages of the filter),
 * "filter_min_query_rows", "max_mean_candidates", "refine" (0 off,
 * 1 on, 2 by measurement: the per-sample refinement in front of the exact stage), "shard_smooth",
 * "csr_densify_below" (see dbgsom_ctx_load_csr), "anchor_seeds" (1, the default: a stateless search of the resident
 * samples in the pruning form takes its seeds from anchor buckets built once per load instead of a seed pre-pass per
 * call; 0: the pre-pass.  Results do not depend on it).
 * Readable besides those: "resident_csr", "resident_nnz", "refined", "shard_epochs", "n_samples", "features", "padded_features", "prototypes",
 * "planes_cached", "planes_used" / "planes_next" (0 = no sweep), "seed_mode", "prune_retry", "hint_valid",
 * "filter_backoff", "plane_hold", "device_bytes", "anchor_builds" (anchor buckets built so far), "anchor_searches" (searches seeded from them), "lean_searches" (of those, epochs in the lean form DBGSOM_ANCHOR_LISTS_ONLY), "hint_bound_searches" (searches that took the hinted pruning bound), "anchor_state" (of
 * the resident samples: 0 none, 1 in use, 2 dropped -- their lists came out longer than the pre-pass's), and the
 * PCIe traffic of the prototypes since the context was created: "w_upload_calls" / "w_upload_bytes"
 * (whole matrices host -> HBM), "w_download_calls" / "w_download_bytes", "w_row_writes", "w_row_reads";
 * and the PCIe traffic of the samples since then: "x_upload_bytes" / "x_upload_calls" (sample rows host -> HBM:
 * dbgsom_ctx_load, dbgsom_ctx_load_csr, the rows of every query handed over as host arrays, chunk by chunk where a
 * call works in chunks) and "x_download_bytes" (per-row results HBM -> host: winners, distances, codes, class
 * probabilities, filled rows).  dbgsom_ctx_load_device and the *_device queries below move neither. */
int dbgsom_ctx_set_option(dbgsom_ctx *ctx, const char *name, int64_t value);
int dbgsom_ctx_get_option(dbgsom_ctx *ctx, const char *name, int64_t *value);
/* the HIP stream (hipStream_t) every call of this context enqueues its work on */
int dbgsom_ctx_stream(dbgsom_ctx *ctx, void **stream);

/* Upload the training samples once (BaseSom.fit's `X`, BaseSom.py:88-114).  x_dtype: what X_host
 * holds; storage: what stays in HBM -- the same, or DBGSOM_BF16 for float32 input rounded to
 * nearest-even bfloat16 on the device (all arithmetic stays float64 on the exactly widened values;
 * an extension, the reference has no bfloat16). */
int dbgsom_ctx_load(dbgsom_ctx *ctx, const void *X_host, int x_dtype, int64_t N, int64_t d,
                    int storage);
/* The same for samples in canonical CSR form (see dbgsom_csr_check, which runs first: DBGSOM_EINVAL on a fault).
 * Below option "csr_densify_below" features (default 1024, 0 = never) the rows are expanded on the device into
 * the ordinary resident form and every call behaves as after dbgsom_ctx_load of the dense matrix.  At and above
 * it the data stays CSR (option "resident_csr" reads 1; nothing of size N x d is allocated): the epoch, the
 * searches and the reductions run the CSR kernels -- all-pairs search, no candidate pruning -- with the results
 * of the dense kernels on the densified matrix bit for bit; everything behind the per-neuron sums is shared.
 * A context with a CSR resident allocates its buffers without head room and runs the smoothing inside the
 * accumulate workspace: it holds less than the CSR arrays, Wt, two W buffers, those two workspaces and 64 bytes per row.
 * Not available on a CSR resident (DBGSOM_ESTATE): dbgsom_ctx_subset_create, dbgsom_ctx_column_sums,
 * dbgsom_ctx_weighted_column_sums; bfloat16 storage is refused (DBGSOM_EINVAL). */
int dbgsom_ctx_load_csr(dbgsom_ctx *ctx, const int64_t *indptr_host, const int32_t *indices_host,
                        const void *data_host, int x_dtype, int64_t N, int64_t d, int64_t nnz);
/* Adopt samples that already live in HBM on the context's device (rows of ldx elements).  Borrowed
 * without a copy when ldx is a multiple of 16 features that covers d and the rows are 16-byte
 * aligned with zeros behind column d; copied (padded) otherwise.  The caller keeps the memory alive
 * and unchanged until another load or dbgsom_ctx_destroy, and has finished writing it. */
int dbgsom_ctx_load_device(dbgsom_ctx *ctx, const void *X_dev, int x_dtype, int64_t N, int64_t d,
                           int64_t ldx);
/* rows of the resident samples, widened to float64 (the four start prototypes of
 * BaseSom._create_som BaseSom.py:419-444 without a host copy of X) */
int dbgsom_ctx_read_samples(dbgsom_ctx *ctx, const int64_t *rows_host, int64_t n, double *out_host);
/* integer class labels of the resident rows (entropy criterion BaseSom.py:547-551) */
int dbgsom_ctx_set_labels(dbgsom_ctx *ctx, const int32_t *y_host, int64_t N);
/* One weight per resident row (float64, finite, >= 0): a row of weight w counts as w copies of that row.
 * With weights attached dbgsom_ctx_epoch, dbgsom_ctx_update, dbgsom_ctx_quantization_error ([sum w dist, sum w]),
 * dbgsom_ctx_topographic_count (summed weight), dbgsom_ctx_node_statistics (hits = sum w, density sums = sum w
 * term) run their weighted forms; the BMU searches do not depend on weights.  In a multi-rank run every rank
 * attaches its own rows' weights.  w_host == NULL detaches.  A wrong N or a negative / non-finite weight is
 * DBGSOM_EINVAL (dbgsom_last_error says which).  dbgsom_ctx_subset_create hands the weights on. */
int dbgsom_ctx_set_sample_weight(dbgsom_ctx *ctx, const double *w_host, int64_t N);
/* sum of the resident rows' weights (this rank's; the number of rows when none are attached) */
int dbgsom_ctx_weight_total(dbgsom_ctx *ctx, double *out_host);
/* weighted column sums of the resident samples in float64 (dbgsom_weighted_column_sums): mean_host == NULL:
 * out_j = sum_i w_i x_ij, else sum_i w_i (x_ij - mean_j)^2; d float64 each */
int dbgsom_ctx_weighted_column_sums(dbgsom_ctx *ctx, const double *mean_host, double *out_host);
/* dbgsom_ctx_class_histogram with weights: hist_host (M x n_classes float64) = summed weights, all ranks */
int dbgsom_ctx_class_histogram_weighted(dbgsom_ctx *ctx, const int64_t *idx_host, int64_t n_classes, int64_t M,
                                        double *hist_host);

/* Lattice hop distances, M x M float64 as nx.floyd_warshall_numpy returns them
 * (BaseSom.py:367,401).  Call again whenever neurons were added. */
int dbgsom_ctx_set_topology(dbgsom_ctx *ctx, const double *hop_host, int64_t M);

/* Sample-sharded runs (one context per GPU / process): `fn` is called once per epoch, between the
 * per-neuron sums and the smoothing, with the fused [S | K | a | E | status] buffer in HBM
 * (count float64 values) and must leave the element-wise SUM over all ranks in it, ordered on
 * `stream` (RCCL: ncclAllReduce(buf, buf, count, ncclDouble, ncclSum, comm, stream)).  The small
 * reductions (QE, TE, node statistics, class histogram) go through it too.  NULL = single rank.
 * Returns 0 on success; anything else makes the call fail with DBGSOM_ECALLBACK. */
typedef int (*dbgsom_allreduce_fn)(void *user, double *buf_dev, int64_t count, void *stream);
int dbgsom_ctx_set_allreduce(dbgsom_ctx *ctx, dbgsom_allreduce_fn fn, void *user);
/* The same collective issued by the library itself: ncclAllReduce(buf, buf, count, ncclDouble, ncclSum)
 * on the context's stream, RCCL over xGMI -- no callback, no interpreter in the epoch (what SURVEY.md 5 /
 * 8(b) asks of the replacement: "the library drives all devices itself").  librccl is resolved at run
 * time (symbols already in the process -- e.g. the copy a loaded PyTorch brought --, else
 * $DBGSOM_RCCL_LIB, else librccl.so[.1] of the system ROCm): the library has no link-time dependency on
 * it and single-GPU callers never load it.
 *   dbgsom_rccl_unique_id     rank 0 makes the 128-byte id (ncclGetUniqueId) and hands it to the other
 *                             ranks by whatever launched them (a file, an environment variable, MPI ...)
 *   dbgsom_rccl_comm_init     every rank, after hipSetDevice / dbgsom_ctx_create on its GPU: a communicator
 *                             of `nranks` (ncclCommInitRank; collective -- all ranks must call it); it
 *                             outlives contexts and is destroyed with dbgsom_rccl_comm_destroy
 *   dbgsom_ctx_set_rccl       the context issues its collective on this communicator (an ncclComm_t as
 *                             void *: one made above, or any the caller owns); NULL detaches
 * It replaces a callback set with dbgsom_ctx_set_allreduce (and the other way round). */
int dbgsom_rccl_unique_id(char *id128);
int dbgsom_rccl_comm_init(const char *id128, int nranks, int rank, void **comm_out);
int dbgsom_rccl_comm_destroy(void *comm);
int dbgsom_ctx_set_rccl(dbgsom_ctx *ctx, void *nccl_comm);
/* The callback seam with everything the epoch can use: one function, three operations on float64 values in
 * HBM, ordered on `stream`, all in place.
 *   DBGSOM_COLL_ALLREDUCE       buf[0 .. count): element-wise SUM over the ranks (as dbgsom_allreduce_fn)
 *   DBGSOM_COLL_REDUCE_SCATTER  buf holds nranks blocks of `count` values; on return block `rank` holds the SUM
 *                               of that block over the ranks (ncclReduceScatter(buf, buf + rank * count, count))
 *   DBGSOM_COLL_ALLGATHER       block `rank` of nranks blocks of `count` values is this rank's; on return every
 *                               block holds its owner's (ncclAllGather(buf + rank * count, buf, count))
 * With the last two (or with RCCL, dbgsom_ctx_set_rccl) the epoch can shard the neighbourhood smoothing
 * (BaseSom.py:509-515) over the ranks: column c of the new prototypes needs column c of the Voronoi sums and
 * nothing else of them, so S is reduce-scattered as column blocks, the small vectors [K | a | E | status]
 * (3 M + 1 values: what growth and convergence are decided from) are all-reduced so that every rank holds the
 * same bits of them, each rank smooths its d / nranks columns, and an all-gather of the blocks leaves the same
 * W' on every rank bit for bit -- the bytes of the all-reduce on the wire, 1 / nranks of the M x M x d product
 * per rank.  Option
 * "shard_smooth": 0 never, 1 whenever the collective can, 2 (default) from ~8 GFLOP of smoothing (2 M^2 d).
 * Results equal the replicated form's bit for bit whenever the reduced sums do (two ranks: always). */
enum { DBGSOM_COLL_ALLREDUCE = 0, DBGSOM_COLL_REDUCE_SCATTER = 1, DBGSOM_COLL_ALLGATHER = 2 };
typedef int (*dbgsom_collective_fn)(void *user, int op, double *buf_dev, int64_t count, void *stream);
int dbgsom_ctx_set_collectives(dbgsom_ctx *ctx, dbgsom_collective_fn fn, void *user, int rank, int nranks);
/* element-wise SUM of `n` host float64 values over the ranks of the context's collective (RCCL or
 * callback; identity for a single rank): what a caller without a communication library of its own needs
 * around the epochs (moments of the data, the start prototypes from rank 0, a barrier, timings) */
int dbgsom_ctx_allreduce_host(dbgsom_ctx *ctx, double *vals_host, int64_t n);

/* The prototypes resident in HBM (M x d float64; `weights_` of the reference).
 *   set_weights   upload all of them
 *   get_weights   which = 0: the resident ones (what an epoch with W_host = NULL consumes);
 *                 which = 1: the other buffer -- after an epoch, the prototypes it consumed (the
 *                 `weights_` snapshot of the reference, quirk Q3); after a FROZEN epoch, its output
 *   read_weight_rows / write_weight_rows: single rows (growth step BaseSom.py:588-861: the
 *                 extrapolated rows are O(d) each); writing at row0 == M appends (M grows) */
int dbgsom_ctx_set_weights(dbgsom_ctx *ctx, const double *W_host, int64_t M);
int dbgsom_ctx_get_weights(dbgsom_ctx *ctx, int which, double *W_host, int64_t M);
int dbgsom_ctx_read_weight_rows(dbgsom_ctx *ctx, int which, const int64_t *rows_host, int64_t n,
                                double *out_host);
int dbgsom_ctx_write_weight_rows(dbgsom_ctx *ctx, int64_t row0, int64_t n, const double *rows_host);

/* _get_winning_neurons on the resident samples.  BaseSom.py:446-464.  W_host = NULL: the resident
 * prototypes.  k = 1 goes through the filtered search where it pays.  dist_host may be NULL (the winners alone
 * come back). */
int dbgsom_ctx_bmu(dbgsom_ctx *ctx, const double *W_host, int64_t M, int k, int round_f32,
                   int64_t *idx_host, double *dist_host);

/* _get_winning_neurons on other samples (predict, SomVQ.py:130-148). */
int dbgsom_ctx_bmu_query(dbgsom_ctx *ctx, const void *Xq_host, int x_dtype, int64_t Nq,
                         int64_t d, const double *W_host, int64_t M, int k, int round_f32,
                         int64_t *idx_host, double *dist_host);

/* The same on rows that already live in HBM on the context's device (rows ldx >= d elements apart, any alignment
 * of the element type): nothing of Xq crosses PCIe in either direction.  The rows are read where they are when they
 * meet the condition of dbgsom_ctx_load_device (d a multiple of 16, ldx == d, 16-byte aligned base) and copied
 * (padded) on the device into the context's query buffer otherwise; the searches, the filtered one included
 * ("filter_min_query_rows"), and their results are those of dbgsom_ctx_bmu_query on the same bytes.  idx_dev /
 * dist_dev: Nq x k device arrays the search writes itself.  The caller has finished writing Xq; the call returns
 * after the context's stream has drained, and no pointer is retained. */
int dbgsom_ctx_bmu_query_device(dbgsom_ctx *ctx, const void *Xq_dev, int x_dtype, int64_t Nq, int64_t d,
                                int64_t ldx, const double *W_host, int64_t M, int k, int round_f32,
                                int64_t *idx_dev, double *dist_dev);

/* the same on CSR samples (the rule of dbgsom_ctx_load_csr decides between the CSR search and expansion) */
int dbgsom_ctx_bmu_query_csr(dbgsom_ctx *ctx, const int64_t *indptr_host, const int32_t *indices_host,
                             const void *data_host, int x_dtype, int64_t Nq, int64_t d, int64_t nnz,
                             const double *W_host, int64_t M, int k, int round_f32, int64_t *idx_host,
                             double *dist_host);

/* ---- query rows with missing entries (csrc/masked.hip) ---------------------------------------------
 * A NaN in a row of X marks a missing entry; prototypes are complete.  With O(x) the observed entries of a
 * row and n_obs their number,
 *   dist(x, w) = sqrt((d / n_obs) * sum_{k in O(x)} (x_k - w_k)^2)
 * (scikit-learn's nan_euclidean_distances; a complete row gets the plain distance).  Direct form in
 * float64 -- t = x_k - w_k, acc = fma(t, t, acc), k ascending -- so a row that equals a prototype on its
 * observed entries is at 0.0 exactly, and a (row, prototype) pair's bits depend on that row and that
 * prototype only.  arg-k-min over j on (sum, j), ties to the lowest j, k in {1, 2}; idx N x k int64, dist
 * N x k float64 as dbgsom_bmu.  There is no float32 rounding of these distances.
 *   X: N x d, DBGSOM_F32 or DBGSOM_F64 (DBGSOM_BF16 is DBGSOM_EINVAL), ldx <= 2^27; W: M x d float64.
 *   A row without any observed entry gets dist = NaN (the context call refuses such rows beforehand).
 * dbgsom_fill_missing writes (x_dtype) W[idx[i * idx_stride]][c] into every NaN position (i, c) of X and
 * leaves everything else as it is (rows whose index is outside [0, M) too).
 * Workspace: 16-byte aligned, contents on entry irrelevant, nothing outside [workspace_dev, workspace_dev +
 * workspace_bytes) is written. */
size_t dbgsom_bmu_masked_workspace_bytes(int x_dtype, int64_t N, int64_t d, int64_t M);
int dbgsom_bmu_masked(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx,
                      const double *W_dev, int64_t M, int64_t ldw, int k, int64_t *idx_dev,
                      double *dist_dev, void *workspace_dev, size_t workspace_bytes, void *stream);
int dbgsom_fill_missing(void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *W_dev,
                        int64_t M, int64_t ldw, const int64_t *idx_dev, int64_t idx_stride, void *stream);
/* The same from host arrays, in chunks of ctx option "masked_chunk_rows" rows on the context's stream.
 * Xfilled_host (Nq x d, x_dtype; may be NULL): the rows with their holes filled from the first winner
 * (filled on the device after each chunk's search).  A row without any observed entry is DBGSOM_EINVAL,
 * found on the host before anything is launched; the message names the first such row. */
int dbgsom_ctx_bmu_query_masked(dbgsom_ctx *ctx, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d,
                                const double *W_host, int64_t M, int k, int64_t *idx_host,
                                double *dist_host, void *Xfilled_host);

/* ---- the distance matrix of a query (csrc/distances.hip) ------------------------------------------------
 * out[i * ldo + j] = the distance from row i of X to prototype j, float64, in the arithmetic of the search bit for
 * bit: sqrt(max((|x_i|^2 + (-2 <x_i, w_j>)) + |w_j|^2, 0)) with each of the three sums a sequential fma chain over
 * the features from +0 (oracle/bmu_chain.c); no float32 rounding.  What dbgsom_bmu returns for a row are this
 * matrix's smallest entries of that row.
 *   X: N x d (DBGSOM_F32 / F64 / BF16), rows ldx >= d elements apart, any d, any element-aligned base; xx / ww:
 *   the squared norms of dbgsom_row_sqnorms; W: M x d float64, contiguous, 1 <= M <= DBGSOM_MAX_PROTOTYPES;
 *   out: rows ldo >= M apart, 8-byte aligned (16-byte stores are used where the base and ldo allow them).
 * Columns [M, ldo) of a row and everything behind row N - 1 are never written.  A NaN in a row gives NaN for
 * that row. */
int dbgsom_distances(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx_dev,
                     const double *W_dev, int64_t M, const double *ww_dev, double *out_dev, int64_t ldo,
                     void *stream);
/* Rows with missing entries (NaN): out[i * ldo + j] = sqrt((d / n_obs) * sum over the observed entries of
 * (x_k - w_k)^2), the chain, the scale and the square root of dbgsom_bmu_masked, whose distances are this
 * matrix's smallest entries per row.  X: DBGSOM_F32 or DBGSOM_F64; W: M x d float64, rows ldw >= d apart; the
 * workspace is that of dbgsom_bmu_masked_workspace_bytes (too small: DBGSOM_ENOMEM).  A row without an
 * observed entry gets NaN. */
int dbgsom_distances_masked(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx,
                            const double *W_dev, int64_t M, int64_t ldw, double *out_dev, int64_t ldo,
                            void *workspace_dev, size_t workspace_bytes, void *stream);
/* The same on a context, each call staging its rows as its dbgsom_ctx_bmu_query* namesake does; W_host: M x d.
 * The host-facing calls (out_host: Nq x M, contiguous) work in chunks of ctx option "distances_chunk_rows" rows
 * (0, the default: as many as keep a chunk's staged result at 256 MiB): a chunk's rows go up, its result comes
 * down.  _device: rows in HBM, read in place under the condition of dbgsom_ctx_load_device and pad-copied on
 * the device otherwise; out_dev (rows ldo >= M apart) is written by the kernel itself and nothing of X or of
 * the result crosses PCIe.  _csr: row chunks are expanded on the device (dbgsom_csr_densify) into the dense
 * kernel, so the result is the dense call's on the expanded rows bit for bit.  _masked: rows with NaN; a row
 * without an observed entry is DBGSOM_EINVAL, found on the host.  Argument errors are reported before any
 * device work. */
int dbgsom_ctx_distances_query(dbgsom_ctx *ctx, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d,
                               const double *W_host, int64_t M, double *out_host);
int dbgsom_ctx_distances_query_device(dbgsom_ctx *ctx, const void *Xq_dev, int x_dtype, int64_t Nq, int64_t d,
                                      int64_t ldx, const double *W_host, int64_t M, double *out_dev,
                                      int64_t ldo);
int dbgsom_ctx_distances_query_csr(dbgsom_ctx *ctx, const int64_t *indptr_host, const int32_t *indices_host,
                                   const void *data_host, int x_dtype, int64_t Nq, int64_t d, int64_t nnz,
                                   const double *W_host, int64_t M, double *out_host);
int dbgsom_ctx_distances_query_masked(dbgsom_ctx *ctx, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d,
                                      const double *W_host, int64_t M, double *out_host);

/* ---- the k nearest prototypes of every row (csrc/kneighbors.hip) -------------------------------------------
 * idx[i * k + t], dist[i * k + t], t = 0 .. k - 1: the k prototypes of row i with the smallest (r_ij, j) in
 * lexicographic order, ascending, where r_ij = max((|x_i|^2 + (-2 <x_i, w_j>)) + |w_j|^2, 0) is the squared value
 * of the search's own fma chain (for rows with missing entries: d / n_obs * sum over the observed (x_k - w_k)^2),
 * and dist = sqrt(r), taken after the selection, float64, no float32 rounding.  The selection is on r: of two
 * distinct r under one square root the smaller comes first whatever the indices.  So columns 0..1 are what
 * dbgsom_bmu reports for k = 2, and dist[i * k + t] is entry idx[i * k + t] of row i of dbgsom_distances, bit for
 * bit.  A pair whose r is not below +inf (NaN, +inf) is never reported; slots left unfilled hold (inf, -1).
 * 1 <= k <= min(M, DBGSOM_MAX_NEIGHBORS).  Argument errors (k, ldr < M, a null pointer, a short workspace:
 * DBGSOM_ENOMEM with both sizes in the message) are reported before any launch.
 *
 * dbgsom_topk_rows: the selection alone on a caller's matrix R of squared values, N rows of M entries ldr >= M
 * apart; idx (int64) and dist (float64) are N x k, contiguous.
 * dbgsom_kneighbors: arguments as dbgsom_distances.  The rows are worked in slabs of slab_rows rows (0: as many,
 * in multiples of 128, as keep a slab at 64 MiB): the squared distances of a slab go into the workspace (rows
 * M rounded up to even apart, ordinary stores), the selection reads them back while they are still in cache.
 * Nothing grows with N x M: dbgsom_kneighbors_workspace_bytes(N, M, slab_rows) is one slab.  The workspace
 * must be 16-byte aligned.
 * dbgsom_kneighbors_masked: rows with missing entries (NaN), arguments as dbgsom_distances_masked; the workspace
 * is that of dbgsom_kneighbors_masked_workspace_bytes (the masked search's for one slab of rows, then the slab).
 * Both workspaces: 16-byte aligned, contents on entry irrelevant, nothing outside [workspace_dev, workspace_dev +
 * workspace_bytes) is written. */
int dbgsom_topk_rows(const double *R_dev, int64_t N, int64_t M, int64_t ldr, int k, int64_t *idx_dev,
                     double *dist_dev, void *stream);
size_t dbgsom_kneighbors_workspace_bytes(int64_t N, int64_t M, int64_t slab_rows);
size_t dbgsom_kneighbors_masked_workspace_bytes(int x_dtype, int64_t N, int64_t d, int64_t M, int64_t slab_rows);
int dbgsom_kneighbors(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx_dev,
                      const double *W_dev, int64_t M, const double *ww_dev, int k, int64_t slab_rows,
                      int64_t *idx_dev, double *dist_dev, void *workspace_dev, size_t workspace_bytes,
                      void *stream);
int dbgsom_kneighbors_masked(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx,
                             const double *W_dev, int64_t M, int64_t ldw, int k, int64_t slab_rows,
                             int64_t *idx_dev, double *dist_dev, void *workspace_dev, size_t workspace_bytes,
                             void *stream);
/* The same on a context, each call staging its rows as its dbgsom_ctx_distances_query* namesake does (chunks of
 * "distances_chunk_rows" host rows, query placement, CSR expanded chunk by chunk, traffic counters, status codes);
 * the slab is ctx option "kneighbors_slab_rows" rows (0, the default: as above).  idx / dist: Nq x k, contiguous;
 * only Nq x k x 16 bytes of result come down per host-facing call.  _device: idx_dev / dist_dev are written by
 * the kernel; nothing of X or of the result crosses PCIe. */
int dbgsom_ctx_kneighbors_query(dbgsom_ctx *ctx, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d,
                                const double *W_host, int64_t M, int k, int64_t *idx_host, double *dist_host);
int dbgsom_ctx_kneighbors_query_device(dbgsom_ctx *ctx, const void *Xq_dev, int x_dtype, int64_t Nq, int64_t d,
                                       int64_t ldx, const double *W_host, int64_t M, int k, int64_t *idx_dev,
                                       double *dist_dev);
int dbgsom_ctx_kneighbors_query_csr(dbgsom_ctx *ctx, const int64_t *indptr_host, const int32_t *indices_host,
                                    const void *data_host, int x_dtype, int64_t Nq, int64_t d, int64_t nnz,
                                    const double *W_host, int64_t M, int k, int64_t *idx_host, double *dist_host);
int dbgsom_ctx_kneighbors_query_masked(dbgsom_ctx *ctx, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d,
                                       const double *W_host, int64_t M, int k, int64_t *idx_host,
                                       double *dist_host);

/* ---- the distortion measure of every row (csrc/distortion.hip) ----------------------------------------------
 * bmu[i] = b, e[i] = sum_j H[b * ldh + j] * r_ij over j < M: b is the index of the smallest (r_ij, j) in
 * lexicographic order among r_ij < +inf, r_ij = max((|x_i|^2 + (-2 <x_i, w_j>)) + |w_j|^2, 0) the squared value of
 * the search's own fma chain (no float32 rounding), H a caller's M x M matrix of float64 neighbourhood factors
 * (rows ldh >= M apart).  The order of the sum is fixed: lane l of 64 adds its terms j = l, l + 64, ... ascending
 * into p_l = p_l + (H[b, j] * r_ij) from +0.0, the product rounded and then the sum (never a fused
 * multiply-add); six rounds m = 1, 2, 4, 8, 16, 32 in which every lane takes p_l + p_(l ^ m) follow, and e is
 * p_0.  Otherwise plain IEEE: a +inf or NaN r_ij enters the sum as it is (0 * inf = NaN).  A row without any
 * r_ij below +inf has (bmu, e) = (-1, NaN).  Argument errors (M, ldr < M, ldh < M, slab_rows < 0, a null or
 * misaligned pointer, a short workspace: DBGSOM_ENOMEM with both sizes in the message) are reported before any
 * launch; N == 0 returns DBGSOM_OK without one.
 *
 * dbgsom_energy_rows: the kernel alone on a caller's matrix R of squared values, N rows of M entries ldr >= M
 * apart; nothing of a row past M is read.  bmu (int64) and e (float64) hold N values each.
 * dbgsom_neighborhood_energy: arguments as dbgsom_kneighbors with H for k: the rows are worked in the same
 * slabs, in the same workspace (dbgsom_kneighbors_workspace_bytes(N, M, slab_rows), 16-byte aligned). */
int dbgsom_energy_rows(const double *R_dev, int64_t N, int64_t M, int64_t ldr, const double *H_dev, int64_t ldh,
                       int64_t *bmu_dev, double *e_dev, void *stream);
int dbgsom_neighborhood_energy(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx,
                               const double *xx_dev, const double *W_dev, int64_t M, const double *ww_dev,
                               const double *H_dev, int64_t ldh, int64_t slab_rows, int64_t *bmu_dev,
                               double *e_dev, void *workspace_dev, size_t workspace_bytes, void *stream);
/* The same on a context, each call staging its rows as its dbgsom_ctx_kneighbors_query* namesake does (chunks,
 * query placement, CSR expanded chunk by chunk, the slab of "kneighbors_slab_rows" rows, status codes).  H_host
 * (M x M, contiguous) goes up once per call and counts as upload traffic; Nq x 16 bytes of result come down per
 * host-facing call.  _device: bmu_dev / e_dev are written by the kernel; nothing of X or of the result crosses
 * PCIe. */
int dbgsom_ctx_distortion_query(dbgsom_ctx *ctx, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d,
                                const double *W_host, int64_t M, const double *H_host, int64_t *bmu_host,
                                double *e_host);
int dbgsom_ctx_distortion_query_device(dbgsom_ctx *ctx, const void *Xq_dev, int x_dtype, int64_t Nq, int64_t d,
                                       int64_t ldx, const double *W_host, int64_t M, const double *H_host,
                                       int64_t *bmu_dev, double *e_dev);
int dbgsom_ctx_distortion_query_csr(dbgsom_ctx *ctx, const int64_t *indptr_host, const int32_t *indices_host,
                                    const void *data_host, int x_dtype, int64_t Nq, int64_t d, int64_t nnz,
                                    const double *W_host, int64_t M, const double *H_host, int64_t *bmu_host,
                                    double *e_host);

/* ---- the k nearest rows to every prototype (csrc/exemplars.hip) ----------------------------------------------
 * The all-pairs search read down its columns: idx[j * k + t], dist[j * k + t] are, for prototype j, the rows i of
 * X with the smallest (r_ij, i) in lexicographic order, ascending, r_ij = max((|x_i|^2 + (-2 <x_i, w_j>)) +
 * |w_j|^2, 0) the squared value dbgsom_kneighbors selects on, and dist = sqrt(r) taken after the selection: equal
 * r go by the lower row, and of two different r under one square root the smaller comes first.  A pair whose r is
 * not below +inf (NaN, +inf) is never reported; slots left unfilled hold (inf, -1).  1 <= k <=
 * DBGSOM_MAX_NEIGHBORS; k may exceed M and N.  With own_cell != 0 row i is a candidate for prototype j only if j
 * is the row's unit, the index of its smallest (r_ij, j) (dbgsom_kneighbors at k = 1); a row without any r below
 * +inf belongs to no unit.  (r, i) is a total order, so the result does not depend on slabs or chunks.
 *
 * dbgsom_topk_cols: the selection alone, as a fold.  R holds N rows of M squared values, ldr >= M apart, with the
 * global row numbers row0 .. row0 + N - 1, row0 >= 0 and row0 + N <= 2^31 - 1.  state_r (M x k float64) and
 * state_i (M x k int64) hold per column the k smallest (r, i) seen so far, ascending, (+inf, -1) in empty slots
 * (dbgsom_topk_cols_init fills them so); after the call they hold the k smallest among what they held and the new
 * rows.  owner_dev is null or N int64 values: row i is folded into column j only if owner[i] == j.  The scratch
 * of one fold is dbgsom_topk_cols_workspace_bytes(N, M, k) bytes, 16-byte aligned; what it held before, and what
 * lies in a row past M, is never read into a result.  N == 0 returns DBGSOM_OK without a launch.
 * dbgsom_exemplars: arguments as dbgsom_kneighbors, idx / dist M x k: it fills the state, runs that call's slab
 * loop (the squared product; with own_cell the selection of dbgsom_topk_rows at k = 1 for the units; the fold)
 * and stores (sqrt(r), i).  The workspace, dbgsom_exemplars_workspace_bytes(N, M, k, slab_rows) bytes, 16-byte
 * aligned, covers the slab, the units of one slab, the fold's scratch and the state.  N == 0 stores (inf, -1).
 * Argument errors (k out of range, ldr < M, slab_rows < 0, row0 + N too large, a null or misaligned pointer; a
 * short workspace: DBGSOM_ENOMEM with both sizes in the message) are reported before any launch.  Both workspaces:
 * contents on entry irrelevant, nothing outside [workspace_dev, workspace_dev + workspace_bytes) is written. */
size_t dbgsom_topk_cols_workspace_bytes(int64_t N, int64_t M, int k);
int dbgsom_topk_cols_init(double *state_r_dev, int64_t *state_i_dev, int64_t M, int k, void *stream);
int dbgsom_topk_cols(const double *R_dev, int64_t N, int64_t M, int64_t ldr, const int64_t *owner_dev, int64_t row0,
                     int k, double *state_r_dev, int64_t *state_i_dev, void *workspace_dev, size_t workspace_bytes,
                     void *stream);
size_t dbgsom_exemplars_workspace_bytes(int64_t N, int64_t M, int k, int64_t slab_rows);
int dbgsom_exemplars(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx_dev,
                     const double *W_dev, int64_t M, const double *ww_dev, int k, int own_cell, int64_t slab_rows,
                     int64_t *idx_dev, double *dist_dev, void *workspace_dev, size_t workspace_bytes, void *stream);
/* The same on a context, each call staging its rows as its dbgsom_ctx_kneighbors_query* namesake does (chunks,
 * query placement, CSR expanded chunk by chunk, the slab of "kneighbors_slab_rows" rows, status codes).  The state
 * lives on the device for the length of the call and every chunk folds into it under its first row's number;
 * nothing per chunk is staged or copied down.  M * k * 16 bytes of result come down, once, per host-facing call.
 * _device: idx_dev / dist_dev are written by the kernel; nothing of X or of the result crosses PCIe.  Nq == 0
 * returns DBGSOM_OK and writes nothing. */
int dbgsom_ctx_exemplars_query(dbgsom_ctx *ctx, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d,
                               const double *W_host, int64_t M, int k, int own_cell, int64_t *idx_host,
                               double *dist_host);
int dbgsom_ctx_exemplars_query_device(dbgsom_ctx *ctx, const void *Xq_dev, int x_dtype, int64_t Nq, int64_t d,
                                      int64_t ldx, const double *W_host, int64_t M, int k, int own_cell,
                                      int64_t *idx_dev, double *dist_dev);
int dbgsom_ctx_exemplars_query_csr(dbgsom_ctx *ctx, const int64_t *indptr_host, const int32_t *indices_host,
                                   const void *data_host, int x_dtype, int64_t Nq, int64_t d, int64_t nnz,
                                   const double *W_host, int64_t M, int k, int own_cell, int64_t *idx_host,
                                   double *dist_host);

/* ---- the rows within a radius of every prototype (csrc/density.hip) ------------------------------------------
 * The all-pairs search read down its columns into integer counts: counts[j * n_radii + t] is the number of rows i
 * with r_ij <= thr[t], r_ij = max((|x_i|^2 + (-2 <x_i, w_j>)) + |w_j|^2, 0) the squared value dbgsom_kneighbors
 * selects on.  The thresholds are squared values, 1 <= n_radii <= DBGSOM_MAX_RADII of them, in any order, passed as
 * given: a caller that means sqrt(r) <= rho passes the largest float64 t with sqrt(t) <= rho (dbgsom_amd.backend.
 * squared_threshold), for which the two conditions are the same.  A pair whose r is NaN is never counted, and a
 * NaN threshold counts nothing.  Integer adds commute: the counts do not depend on slabs, chunks or the order in
 * which the wavefronts arrive.
 *
 * dbgsom_range_count_cols: the fold alone.  R holds N <= 2^31 - 1 rows of M squared values, ldr >= M apart; what
 * lies in a row past M is never read.  counts_dev (M x n_radii int64) is ADDED to: the caller zeroes it.  N == 0
 * returns DBGSOM_OK without a launch.
 * dbgsom_range_counts: arguments as dbgsom_kneighbors with thr_dev / n_radii for k and counts_dev (M x n_radii
 * int64) for the result: it zeroes the counts and runs that call's slab loop with the fold behind the squared
 * product.  The workspace, dbgsom_range_counts_workspace_bytes(N, M, slab_rows) bytes, 16-byte aligned, is the
 * slab.  N == 0 stores zeros.  Argument errors (n_radii out of range, ldr < M, slab_rows < 0, a null or misaligned
 * pointer; a short workspace: DBGSOM_ENOMEM with both sizes in the message) are reported before anything touches
 * the device.  Workspace contents on entry are irrelevant; nothing outside [workspace_dev, workspace_dev +
 * workspace_bytes) is written. */
#define DBGSOM_MAX_RADII 32
int dbgsom_range_count_cols(const double *R_dev, int64_t N, int64_t M, int64_t ldr, const double *thr_dev, int n_radii,
                            int64_t *counts_dev, void *stream);
size_t dbgsom_range_counts_workspace_bytes(int64_t N, int64_t M, int64_t slab_rows);
int dbgsom_range_counts(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx_dev,
                        const double *W_dev, int64_t M, const double *ww_dev, const double *thr_dev, int n_radii,
                        int64_t slab_rows, int64_t *counts_dev, void *workspace_dev, size_t workspace_bytes,
                        void *stream);
/* The same on a context, each call staging its rows as its dbgsom_ctx_exemplars_query* namesake does (chunks,
 * query placement, CSR expanded chunk by chunk, the slab of "kneighbors_slab_rows" rows, status codes).  The
 * thresholds (thr_host, n_radii float64) go up once and count as upload traffic; the counts live on the device for
 * the length of the call and every chunk folds into them; nothing per chunk is staged or copied down.  M * n_radii
 * * 8 bytes of result come down, once, per host-facing call.  _device: counts_dev is written on the device; nothing
 * of X or of the result crosses PCIe.  Nq == 0 returns DBGSOM_OK and writes nothing. */
int dbgsom_ctx_range_counts_query(dbgsom_ctx *ctx, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d,
                                  const double *W_host, int64_t M, const double *thr_host, int n_radii,
                                  int64_t *counts_host);
int dbgsom_ctx_range_counts_query_device(dbgsom_ctx *ctx, const void *Xq_dev, int x_dtype, int64_t Nq, int64_t d,
                                         int64_t ldx, const double *W_host, int64_t M, const double *thr_host,
                                         int n_radii, int64_t *counts_dev);
int dbgsom_ctx_range_counts_query_csr(dbgsom_ctx *ctx, const int64_t *indptr_host, const int32_t *indices_host,
                                      const void *data_host, int x_dtype, int64_t Nq, int64_t d, int64_t nnz,
                                      const double *W_host, int64_t M, const double *thr_host, int n_radii,
                                      int64_t *counts_host);

/* ---- the map as an isotropic Gaussian mixture (csrc/mixture.hip) ---------------------------------------------
 * Prototypes w_j, log-priors a_j (logprior, M float64; -inf allowed: a unit without mass) and c = 1 / (2 h^2) >= 0
 * for one bandwidth h.  With r_ij = max((|x_i|^2 + (-2 <x_i, w_j>)) + |w_j|^2, 0) the squared value
 * dbgsom_kneighbors selects on, row i has
 *   t_j   = a_j - (c * r_ij)      the product rounded, then the difference rounded (never a fused multiply-add)
 *   (T,b) = the largest t_j, lowest j among equals, over t_j > -inf and not NaN
 *   s_j   = exp(t_j - T)          S = sum_j s_j          Q_v = sum_j (s_j * Y[j * ldy + v])
 *   unit[i] = b     lse[i] = T + log(S)     q[i * ldq + v] = Q_v / S,   v = 0 .. n_values - 1
 * so lse - (d / 2) log(2 pi h^2) is the log-density of the row, b its MAP unit (the unit of dbgsom_kneighbors at
 * k = 1 under equal priors) and q the posterior mean of the per-unit values Y (M x n_values float64, rows ldy
 * apart).  The order of the sums is that of dbgsom_energy_rows: lane l of 64 adds its terms j = l, l + 64, ...
 * ascending from +0.0 -- in Q the product rounded and then the sum --, then six rounds m = 1, 2, 4, 8, 16, 32 in
 * which every lane takes p_l + p_(l ^ m).  exp and log are the device library's float64 functions; Q_v / S is one
 * division per row and value.  Otherwise plain IEEE: r = +inf gives s = 0; a NaN t_j is never the maximum but
 * enters the sums as it is, so that row's lse and q are NaN.  A row without any t_j above -inf has (unit, lse, q)
 * = (-1, NaN, NaN).  0 <= n_values <= DBGSOM_MAX_MIXTURE_VALUES; with n_values == 0 (density only) Y_dev and
 * q_dev are null.  Argument errors (M, n_values, ldr < M, ldy < n_values, ldq < n_values, c negative or NaN,
 * slab_rows < 0, a null or misaligned pointer, a short workspace: DBGSOM_ENOMEM with both sizes in the message)
 * are reported before any launch; N == 0 returns DBGSOM_OK without one.
 *
 * dbgsom_mixture_rows: the kernel alone on a caller's matrix R of squared values, N rows of M entries ldr >= M
 * apart; nothing of a row past M, of a row of Y past n_values or of a row of q past n_values is touched.
 * dbgsom_mixture: arguments as dbgsom_neighborhood_energy: the rows are worked in the same slabs, in the same
 * workspace (dbgsom_kneighbors_workspace_bytes(N, M, slab_rows): the slab is sized by that one function, 16-byte
 * aligned, contents on entry irrelevant). */
#define DBGSOM_MAX_MIXTURE_VALUES 16
int dbgsom_mixture_rows(const double *R_dev, int64_t N, int64_t M, int64_t ldr, const double *logprior_dev, double c,
                        const double *Y_dev, int n_values, int64_t ldy, int64_t *unit_dev, double *lse_dev,
                        double *q_dev, int64_t ldq, void *stream);
int dbgsom_mixture(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *xx_dev,
                   const double *W_dev, int64_t M, const double *ww_dev, const double *logprior_dev, double c,
                   const double *Y_dev, int n_values, int64_t ldy, int64_t slab_rows, int64_t *unit_dev,
                   double *lse_dev, double *q_dev, int64_t ldq, void *workspace_dev, size_t workspace_bytes,
                   void *stream);
/* The same on a context, each call staging its rows as its dbgsom_ctx_distortion_query* namesake does (chunks,
 * query placement, CSR expanded chunk by chunk, the slab of "kneighbors_slab_rows" rows, status codes).
 * logprior_host (M) and Y_host (M x n_values, contiguous) go up once per call and count as upload traffic; q is
 * Nq x n_values, contiguous; Nq x (16 + 8 n_values) bytes of result come down per host-facing call.  _device:
 * unit_dev / lse_dev / q_dev are written by the kernel; nothing of X or of the result crosses PCIe. */
int dbgsom_ctx_mixture_query(dbgsom_ctx *ctx, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d,
                             const double *W_host, int64_t M, const double *logprior_host, double c,
                             const double *Y_host, int n_values, int64_t *unit_host, double *lse_host,
                             double *q_host);
int dbgsom_ctx_mixture_query_device(dbgsom_ctx *ctx, const void *Xq_dev, int x_dtype, int64_t Nq, int64_t d,
                                    int64_t ldx, const double *W_host, int64_t M, const double *logprior_host,
                                    double c, const double *Y_host, int n_values, int64_t *unit_dev,
                                    double *lse_dev, double *q_dev);
int dbgsom_ctx_mixture_query_csr(dbgsom_ctx *ctx, const int64_t *indptr_host, const int32_t *indices_host,
                                 const void *data_host, int x_dtype, int64_t Nq, int64_t d, int64_t nnz,
                                 const double *W_host, int64_t M, const double *logprior_host, double c,
                                 const double *Y_host, int n_values, int64_t *unit_host, double *lse_host,
                                 double *q_host);

/* ---- weighted geodesics over the lattice and the combined error (csrc/geodesics.hip) -------------------------
 * The combined error of Kaski and Lagus (1996): e_i = d1_i + G[b1_i, b2_i], the distance of row i to its best
 * matching unit plus the length of the shortest path along the map from that unit to the second-best one, a
 * lattice edge being as long as its two prototypes are apart in the input space.  Euclidean metric, complete rows.
 *
 * Edge length.  len(a, b) = sqrt(s) with s = 0 and then, for k ascending, t = W[a, k] - W[b, k], p = t * t,
 * s = s + p: the subtraction, the product and the sum each rounded on their own in float64 (never a fused
 * multiply-add), so len(a, b) == len(b, a) bit for bit.
 * Geodesic.  G[s, t] is the minimum over lattice paths s = v0, v1, .., vn = t of the left fold
 * ((0 + len(v0, v1)) + len(v1, v2)) + ... in float64; G[s, s] = 0, and G[s, t] = +inf when no path exists.
 * Rounded addition of a non-negative length is monotone, so this minimum is the unique least fixed point of
 * dist[v] = min(dist[v], dist[u] + len(u, v)) from dist[s] = 0: every relaxation order ends in the same bits.
 * G[s, t] and G[t, s] fold from different ends and differ in their last bits for most pairs; row s is the fold
 * from s, and nothing is symmetrised.
 * Combined error.  e_i = d1_i + G[b1_i * ldg + b2_i], one rounded addition; NaN for a row with index -1 in
 * either slot.
 *
 * dbgsom_edge_lengths: E undirected edges as int32 pairs (a, b) -> E float64 lengths over W (M rows of d values,
 * ldw >= d apart).  An index outside [0, M) reads nothing, leaves NaN and is DBGSOM_ERANGE.  Blocking.
 * dbgsom_geodesics: row r of G (S rows, ldg >= M apart) is the vector of source sources[r]; sources_dev == NULL
 * means all M sources in order, and then S == M.  One source per workgroup with its vector in LDS (8 M bytes),
 * relaxed by a push over the edge list with 64-bit unsigned atomic minima (non-negative doubles and +inf order
 * as their bit patterns) until a round lowers nothing, at most M - 1 rounds.  Self-loops are ignored, repeated
 * edges are harmless, degree is not bounded, +inf is a legal length and connects nothing.  An edge or source index
 * outside [0, M) is DBGSOM_ERANGE (nothing is read or written through it), a length that is NaN or negative is
 * DBGSOM_EINVAL; the result is then unspecified.  The workspace holds dbgsom_geodesics_workspace_bytes(M, E) bytes
 * (0 for a bad M or E), 256-byte aligned; what it holds on entry does not matter, and nothing outside
 * [workspace_dev, workspace_dev + workspace_bytes) is written.  Blocking: the status word is read back.
 * dbgsom_combined_error_rows: idx2 holds N pairs (b1, b2) of int64, dist N rows ldd >= 1 apart whose first
 * value is d1.  An index outside [0, M) other than -1 reads nothing, leaves NaN and is DBGSOM_ERANGE.  Blocking.
 * Argument errors (null pointers, M < 1 or M > DBGSOM_MAX_PROTOTYPES, E < 0, ldg < M, a short workspace:
 * DBGSOM_ENOMEM, a misaligned one) are reported before any launch. */
int dbgsom_edge_lengths(const double *W_dev, int64_t M, int64_t d, int64_t ldw, const int32_t *edges_dev, int64_t E,
                        double *len_dev, void *stream);
size_t dbgsom_geodesics_workspace_bytes(int64_t M, int64_t E);
int dbgsom_geodesics(const int32_t *edges_dev, const double *len_dev, int64_t E, int64_t M,
                     const int32_t *sources_dev, int64_t S, double *G_dev, int64_t ldg, void *workspace_dev,
                     size_t workspace_bytes, void *stream);
int dbgsom_combined_error_rows(const int64_t *idx2_dev, const double *dist_dev, int64_t ldd, int64_t N,
                               const double *G_dev, int64_t ldg, int64_t M, double *e_dev, void *stream);
/* The same on a context.  dbgsom_ctx_geodesics: W_host (M x d, contiguous) and edges_host (E int32 pairs) go up,
 * the whole M x M matrix comes down into G_host.  dbgsom_ctx_combined_error_query*: the rows and W_host are taken
 * as the dbgsom_ctx_bmu_query* namesake takes them (CSR rows are expanded on the device chunk by chunk); each call
 * runs G over all sources once into a buffer the context owns, then, chunk by chunk ("distances_chunk_rows"), the
 * all-pairs k = 2 search of dbgsom_ctx_bmu_query with round_f32 = 0 (the query search takes its filtered form at
 * k = 1 only) and the rows kernel behind it: pairs and distances stay in HBM.  idx2 is Nq x 2 int64 (best, second),
 * e Nq float64; M >= 2.  Host results (24 bytes per row) go to host memory; _device: both are device arrays the
 * kernels write, and nothing but W and the edges crosses PCIe. */
int dbgsom_ctx_geodesics(dbgsom_ctx *ctx, const double *W_host, int64_t M, int64_t d, const int32_t *edges_host,
                         int64_t E, double *G_host);
int dbgsom_ctx_combined_error_query(dbgsom_ctx *ctx, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d,
                                    const double *W_host, int64_t M, const int32_t *edges_host, int64_t E,
                                    int64_t *idx2_host, double *e_host);
int dbgsom_ctx_combined_error_query_device(dbgsom_ctx *ctx, const void *Xq_dev, int x_dtype, int64_t Nq, int64_t d,
                                           int64_t ldx, const double *W_host, int64_t M, const int32_t *edges_host,
                                           int64_t E, int64_t *idx2_dev, double *e_dev);
int dbgsom_ctx_combined_error_query_csr(dbgsom_ctx *ctx, const int64_t *indptr_host, const int32_t *indices_host,
                                        const void *data_host, int x_dtype, int64_t Nq, int64_t d, int64_t nnz,
                                        const double *W_host, int64_t M, const int32_t *edges_host, int64_t E,
                                        int64_t *idx2_host, double *e_host);

/* ---- fit on rows with missing entries (csrc/masked_fit.hip, csrc/smooth.hip) ---------------------------
 * One epoch on prototypes W (M x d, complete), hop matrix and sigma, NaN marking a missing entry of X:
 *   1. (dist_i, win_i): the masked search above with k = 1 -- every row goes through it, complete rows
 *      included; kw_i = 1 - sqrt(1 - exp(-gamma dist_i^2)) (dbgsom_exp_similarity).
 *   2. per neuron j and feature c, over the rows with win_i = j whose entry c is observed:
 *        S_jc = sum kw_i x_ic,  K_jc = sum kw_i,  A_jc = their number;
 *      per neuron over all of its rows: a_j = their number, E_j = sum dist_i.
 *   3. centres C_jc = S_jc / K_jc where A_jc > 0.
 *   4. h = exp(-(hop^2 / (2 sigma^2))),  W'_jc = sum_l h_jl A_lc C_lc / sum_l h_jl A_lc over the l with
 *      A_lc > 0; where that denominator is 0 (a disconnected lattice, underflow) W'_jc = W_jc bit for bit.
 *      Always the aligned form (row = neuron id; on complete rows: DBGSOM_CENTRES_ALIGNED of dbgsom_smooth);
 *      the compacted layout has no per-feature meaning and is not offered.
 *   5. change_total = sum_j |W_j - W'_j|_2; the epoch's errors are E, its activations a.
 *
 * dbgsom_accumulate_masked is step 2 with the caller's winners, sample kernel values and distances:
 *   sums_dev: M (3 d + 2) float64 = [S (M x d) | K (M x d) | A (M x d) | a (M) | E (M)], every part a sum over
 *   rows (all-reducible).  Stable counting sort by winner, chunks of <= 128 rows summed in list order, chunk
 *   partials in chunk order, groups in group order: bitwise reproducible, independent of the grid, no
 *   floating-point atomics.  A (neuron, feature) nobody observed keeps exact zeros in S, K and A; A and a are
 *   exact integers.  Only the first d columns of a row are data (whatever sits between d and ldx is never
 *   added).  X: DBGSOM_F32 or DBGSOM_F64 (DBGSOM_BF16 is DBGSOM_EINVAL), any ldx >= d, any alignment of its
 *   element type (16-byte aligned rows take the vector loads).  A winner outside [0, M) sets *status_dev (may
 *   be NULL) to 1 and its row is skipped, as in dbgsom_accumulate.
 * Both workspaces (dbgsom_accumulate_masked, dbgsom_smooth_masked): 256-byte aligned, contents on entry irrelevant,
 * nothing outside [workspace_dev, workspace_dev + workspace_bytes) is written.
 * dbgsom_smooth_masked is steps 3-5 on such sums: hop_dev M x M float32, W_old / W_new M x d float64 (no
 * padding; W_new must not alias W_old), change_total_dev one float64. */
size_t dbgsom_accumulate_masked_workspace_bytes(int64_t N, int64_t d, int64_t M);
int dbgsom_accumulate_masked(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx,
                             const int64_t *idx_dev, const double *kw_dev, const double *dist_dev, int64_t M,
                             double *sums_dev, int32_t *status_dev, void *workspace_dev, size_t workspace_bytes,
                             void *stream);
size_t dbgsom_smooth_masked_workspace_bytes(int64_t M, int64_t d);
int dbgsom_smooth_masked(const double *sums_dev, int64_t M, int64_t d, const float *hop_dev, double sigma,
                         const double *W_old_dev, double *W_new_dev, double *change_total_dev,
                         void *workspace_dev, size_t workspace_bytes, void *stream);
/* Context level.  dbgsom_ctx_set_option(ctx, "incomplete", 1) after a dbgsom_ctx_load marks the resident rows
 * as rows with missing entries (the next load clears it; dense DBGSOM_F32 / DBGSOM_F64 residents only, no
 * sample weights, one rank -- DBGSOM_EINVAL otherwise).  What depends on the rows alone is made then, once
 * per load: n_obs per row and, for float32 rows, their float64 copy (N x d x 8 bytes of HBM).  From then on
 * every ordinary context call that would compute on the rows (dbgsom_ctx_epoch, _bmu, _update, _partition,
 * _subset_create, _column_sums, _weighted_column_sums, _quantization_error, _topographic_count,
 * _node_statistics, _set_hint, _read_anchors, and the filter planes and anchors behind them) returns
 * DBGSOM_EINVAL with a message instead of a result computed from NaN.  In their place:
 *   dbgsom_ctx_bmu_masked    the masked search of the resident rows, k in {1, 2}; idx / dist N x k
 *   dbgsom_ctx_epoch_masked  steps 1-5, one call per epoch.  W_host, W_new_host: M x d; the prototypes are
 *                            handed over with every call (nothing stays resident between masked epochs);
 *                            errors_host / activations_host: M; idx_host / dist_host (N each) may be NULL.
 *                            Needs dbgsom_ctx_set_topology for M neurons (DBGSOM_ESTATE otherwise).
 * Both return DBGSOM_EINVAL on rows not marked incomplete (CSR and bfloat16 residents never are), with
 * sample weights attached, or with more than one rank. */
int dbgsom_ctx_bmu_masked(dbgsom_ctx *ctx, const double *W_host, int64_t M, int k, int64_t *idx_host,
                          double *dist_host);
int dbgsom_ctx_epoch_masked(dbgsom_ctx *ctx, const double *W_host, int64_t M, double gamma, double sigma,
                            double *W_new_host, double *change_total_host, double *errors_host,
                            double *activations_host, int64_t *idx_host, double *dist_host);

/* ---- metric="manhattan" (csrc/manhattan.hip) ---------------------------------------------------------
 * dist(x, w) = sum_k |x_k - w_k| in float64, one accumulator per (row, prototype) pair, k ascending:
 * t = x_k - w_k; acc = acc + |t|.  float32 rows are widened exactly first; there is no square root and no
 * clamp.  Winners are the lexicographic minimum on (dist, index); a pair whose distance is not below +inf (a
 * NaN or an infinity in the row) is never reported: index -1, distance +inf.  A pair's bits depend on that row
 * and that prototype only -- not on the batch, the grid, the chunk or the slab.
 * Device level: the arguments of the _masked namesakes above (X DBGSOM_F32 / DBGSOM_F64 with ldx >= d, W
 * float64 with ldw >= d; k in {1, 2} for the search, 1 <= k <= DBGSOM_MAX_NEIGHBORS for the selection, which
 * stores the distance it selected on).  Workspace: dbgsom_bmu_manhattan_workspace_bytes (search and matrix),
 * dbgsom_kneighbors_manhattan_workspace_bytes; both 16-byte aligned, contents on entry irrelevant, nothing outside
 * [workspace_dev, workspace_dev + workspace_bytes) is written; a short one is DBGSOM_ENOMEM. */
size_t dbgsom_bmu_manhattan_workspace_bytes(int x_dtype, int64_t N, int64_t d, int64_t M);
int dbgsom_bmu_manhattan(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *W_dev,
                         int64_t M, int64_t ldw, int k, int64_t *idx_dev, double *dist_dev, void *workspace_dev,
                         size_t workspace_bytes, void *stream);
int dbgsom_distances_manhattan(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx,
                               const double *W_dev, int64_t M, int64_t ldw, double *out_dev, int64_t ldo,
                               void *workspace_dev, size_t workspace_bytes, void *stream);
size_t dbgsom_kneighbors_manhattan_workspace_bytes(int x_dtype, int64_t N, int64_t d, int64_t M, int64_t slab_rows);
int dbgsom_kneighbors_manhattan(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx,
                                const double *W_dev, int64_t M, int64_t ldw, int k, int64_t slab_rows,
                                int64_t *idx_dev, double *dist_dev, void *workspace_dev, size_t workspace_bytes,
                                void *stream);
/* Context level, resident rows.  dbgsom_ctx_bmu_manhattan: the search of the resident rows, k in {1, 2}, idx /
 * dist N x k to the host.  dbgsom_ctx_epoch_manhattan: that search with k = 1 in front of the sums and the
 * smoothing of dbgsom_ctx_epoch (same kernels, `layout` honoured, same outputs); the prototypes (M x d) are
 * handed over with every call; idx_host / dist_host (N each) may be NULL; needs dbgsom_ctx_set_topology for M
 * neurons (DBGSOM_ESTATE otherwise).  Both return DBGSOM_EINVAL, with the reason in the message, on CSR
 * residents, bfloat16 storage, rows marked incomplete, attached sample weights and more than one rank. */
int dbgsom_ctx_bmu_manhattan(dbgsom_ctx *ctx, const double *W_host, int64_t M, int k, int64_t *idx_host,
                             double *dist_host);
int dbgsom_ctx_epoch_manhattan(dbgsom_ctx *ctx, const double *W_host, int64_t M, double gamma, double sigma,
                               int layout, double *W_new_host, double *change_total_host, double *errors_host,
                               double *activations_host, int64_t *idx_host, double *dist_host);
/* Context level, queries: host rows (Nq x d, contiguous) go up in chunks -- "masked_chunk_rows" rows for the
 * search, "distances_chunk_rows" for the matrix and the selection -- and only the results come down; the traffic
 * counters count both.  _device: rows in HBM, ldx >= d elements apart, read where they are; the results are
 * device arrays the kernels write (out_dev rows ldo >= M apart); nothing of X or of the result crosses PCIe. */
int dbgsom_ctx_bmu_query_manhattan(dbgsom_ctx *ctx, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d,
                                   const double *W_host, int64_t M, int k, int64_t *idx_host, double *dist_host);
int dbgsom_ctx_bmu_query_manhattan_device(dbgsom_ctx *ctx, const void *Xq_dev, int x_dtype, int64_t Nq, int64_t d,
                                          int64_t ldx, const double *W_host, int64_t M, int k, int64_t *idx_dev,
                                          double *dist_dev);
int dbgsom_ctx_distances_query_manhattan(dbgsom_ctx *ctx, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d,
                                         const double *W_host, int64_t M, double *out_host);
int dbgsom_ctx_distances_query_manhattan_device(dbgsom_ctx *ctx, const void *Xq_dev, int x_dtype, int64_t Nq,
                                                int64_t d, int64_t ldx, const double *W_host, int64_t M,
                                                double *out_dev, int64_t ldo);
int dbgsom_ctx_kneighbors_query_manhattan(dbgsom_ctx *ctx, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d,
                                          const double *W_host, int64_t M, int k, int64_t *idx_host,
                                          double *dist_host);
int dbgsom_ctx_kneighbors_query_manhattan_device(dbgsom_ctx *ctx, const void *Xq_dev, int x_dtype, int64_t Nq,
                                                 int64_t d, int64_t ldx, const double *W_host, int64_t M, int k,
                                                 int64_t *idx_dev, double *dist_dev);

/* ---- metric="cosine" (csrc/cosine.hip; the cosine forms of the kernels of bmu.hip, bmu_dma.hip, distances.hip) ----
 * With a_ij = <x_i, w_j>, q_i = |x_i|^2 and p_j = |w_j|^2 the sequential chains of dbgsom_bmu and
 * dbgsom_row_sqnorms (acc = fma(x_k, w_k, acc), k ascending, float32 rows widened exactly), in float64, every
 * operation rounded on its own:
 *     inv(t) = 0 if t == 0;  1 / sqrt(t) if 0 < t < +inf;  NaN otherwise     (sqrt, then the division)
 *     u_i = inv(q_i), v_j = inv(p_j);   s_ij = (a_ij * u_i) * v_j;   c_ij = 1 - s_ij  (never a fused multiply-add)
 *     c > 2 -> 2;  not (c > 0) -> 0, except that NaN stays NaN
 * No square root of c, no float32 rounding.  Winners are the lexicographic minimum on (c, index); a pair whose c
 * is not below +inf (NaN or an infinity in the row, a squared norm that overflows) is never reported: index -1,
 * distance +inf; the matrix keeps its NaN.  A zero row, or one whose squared norm underflows to 0, is at distance
 * 1 from every prototype (the lowest index wins).  A pair's bits depend on that row and that prototype only --
 * not on the batch, the grid, the chunk or the slab.
 * Device level: the arguments of the Euclidean namesakes with u_dev for xx_dev, v_dev for ww_dev and without
 * round_f32; X DBGSOM_F32 / DBGSOM_F64 (DBGSOM_BF16: DBGSOM_EINVAL).  dbgsom_inv_norms: out[i] = inv(sq[i]) for n
 * values (both 8-byte aligned; in place is not supported).  dbgsom_kneighbors_cosine stores the distance it selected
 * on; its workspace is that of dbgsom_kneighbors (16-byte aligned, contents on entry irrelevant, nothing outside
 * [workspace_dev, workspace_dev + workspace_bytes) is written; a short one is DBGSOM_ENOMEM). */
int dbgsom_inv_norms(const double *sq_dev, int64_t n, double *out_dev, void *stream);
int dbgsom_bmu_cosine(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *u_dev,
                      const double *W_dev, int64_t M, const double *v_dev, int k, int64_t *idx_dev,
                      double *dist_dev, void *stream);
int dbgsom_distances_cosine(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *u_dev,
                            const double *W_dev, int64_t M, const double *v_dev, double *out_dev, int64_t ldo,
                            void *stream);
size_t dbgsom_kneighbors_cosine_workspace_bytes(int64_t N, int64_t M, int64_t slab_rows);
int dbgsom_kneighbors_cosine(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *u_dev,
                             const double *W_dev, int64_t M, const double *v_dev, int k, int64_t slab_rows,
                             int64_t *idx_dev, double *dist_dev, void *workspace_dev, size_t workspace_bytes,
                             void *stream);
/* Context level, resident rows.  dbgsom_ctx_bmu_cosine: the search of the resident rows, k in {1, 2}, idx / dist
 * N x k to the host.  dbgsom_ctx_epoch_cosine: that search with k = 1 in front of the sums and the smoothing of
 * dbgsom_ctx_epoch (same kernels, `layout` honoured, same outputs); the prototypes (M x d) are handed over with
 * every call, hint and bound are dropped, the search policy is not consulted; idx_host / dist_host (N each) may
 * be NULL; needs dbgsom_ctx_set_topology for M neurons (DBGSOM_ESTATE otherwise).  u of the resident rows is made
 * once per load, on the first of these calls, and stays in HBM (8 N bytes, counted in "device_bytes").  Both
 * return DBGSOM_EINVAL, with the reason in the message, on CSR residents, bfloat16 storage, rows marked
 * incomplete, attached sample weights and more than one rank. */
int dbgsom_ctx_bmu_cosine(dbgsom_ctx *ctx, const double *W_host, int64_t M, int k, int64_t *idx_host,
                          double *dist_host);
int dbgsom_ctx_epoch_cosine(dbgsom_ctx *ctx, const double *W_host, int64_t M, double gamma, double sigma,
                            int layout, double *W_new_host, double *change_total_host, double *errors_host,
                            double *activations_host, int64_t *idx_host, double *dist_host);
/* Context level, queries: as the _manhattan queries above -- host rows (Nq x d, contiguous) go up in chunks of
 * "masked_chunk_rows" rows for the search and "distances_chunk_rows" for the matrix and the selection, only the
 * results come down, the traffic counters count both.  _device: rows in HBM, ldx >= d elements apart, read where
 * they are (no copy, whatever ldx and the alignment); the results are device arrays the kernels write (out_dev
 * rows ldo >= M apart); nothing of X or of the result crosses PCIe. */
int dbgsom_ctx_bmu_query_cosine(dbgsom_ctx *ctx, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d,
                                const double *W_host, int64_t M, int k, int64_t *idx_host, double *dist_host);
int dbgsom_ctx_bmu_query_cosine_device(dbgsom_ctx *ctx, const void *Xq_dev, int x_dtype, int64_t Nq, int64_t d,
                                       int64_t ldx, const double *W_host, int64_t M, int k, int64_t *idx_dev,
                                       double *dist_dev);
int dbgsom_ctx_distances_query_cosine(dbgsom_ctx *ctx, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d,
                                      const double *W_host, int64_t M, double *out_host);
int dbgsom_ctx_distances_query_cosine_device(dbgsom_ctx *ctx, const void *Xq_dev, int x_dtype, int64_t Nq,
                                             int64_t d, int64_t ldx, const double *W_host, int64_t M,
                                             double *out_dev, int64_t ldo);
int dbgsom_ctx_kneighbors_query_cosine(dbgsom_ctx *ctx, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d,
                                       const double *W_host, int64_t M, int k, int64_t *idx_host,
                                       double *dist_host);
int dbgsom_ctx_kneighbors_query_cosine_device(dbgsom_ctx *ctx, const void *Xq_dev, int x_dtype, int64_t Nq,
                                              int64_t d, int64_t ldx, const double *W_host, int64_t M, int k,
                                              int64_t *idx_dev, double *dist_dev);

/* ---- sparse coding: BaseSom.transform / SomClassifier.predict_proba (BaseSom.py:241-268,
 * SomClassifier.py:178-220) ------------------------------------------------------------------------
 * scikit-learn's SparseCoder(dictionary=normalize(W), transform_algorithm="lasso_lars",
 * positive_code=True, transform_alpha=0).transform(normalize(Xq)): one non-negative LARS-lasso path
 * per query row over the Gram matrix of the normalised prototypes (csrc/sparse_code.hip).
 *   code  Nq x M, or NULL
 *   proba Nq x C = (code P) / rowsum(code P) (P: M x C class frequencies), or NULL; a zero code row
 *         gives a NaN row, as the reference's division does
 *   cap   active-set size solved in LDS (0 = the library's 64); rows whose active set grows past it
 *         are solved again by the overflow pass with the factor in the workspace (same results)
 *   counts (device) DBGSOM_SC_COUNTS uint64 counters, ADDED to (zero them before the first call):
 *         [rows, LARS iterations, max iterations of a row, drops, degenerate regressors skipped,
 *          lasso early stops (alpha grew), non-finite AA retries, rows of the overflow pass,
 *          largest active set, steps that dropped more than one prototype at once, G rows read
 *          by corr_eq_dir (sum over the iterations of the active-set size)]
 *   workspace 256-byte aligned, contents on entry irrelevant (the call clears the four list counters it reads),
 *         nothing outside [workspace_dev, workspace_dev + workspace_bytes) is written; a short or misaligned one is
 *         DBGSOM_EINVAL before anything is launched */
#define DBGSOM_SC_COUNTS 11
size_t dbgsom_sparse_code_workspace_bytes(int64_t Nq, int64_t d, int64_t M, int max_iter);
int dbgsom_sparse_code(const void *Xq_dev, int x_dtype, int64_t Nq, int64_t d, int64_t ldx,
                       const double *W_dev, int64_t M, int64_t ldw, int max_iter, int cap,
                       const double *P_dev, int64_t C, double *code_dev, double *proba_dev,
                       uint64_t *counts_dev, void *workspace_dev, size_t workspace_bytes,
                       void *stream);
/* diagnostics: per-stage HIP-event timing of dbgsom_sparse_code (calls become blocking while it is on);
 * enabling or disabling resets the sums.  ms5 = summed ms of [normalise W + Gram GEMM, normalise the
 * queries + Cov GEMM, LARS (LDS path), first overflow pass, second overflow pass] */
int dbgsom_sparse_code_timing(int enable);
int dbgsom_sparse_code_stage_ms(double *ms5);
/* The same from host arrays, in chunks of ctx option "sc_chunk_rows" query rows (workspace stays
 * bounded); option "sc_cap" is the `cap` above.  Xq_host: Nq x d, DBGSOM_F32 or DBGSOM_F64;
 * W_host = NULL: the resident prototypes; P_host: M x C (needed when proba_host is given);
 * code_host / proba_host may be NULL; counts_host[DBGSOM_SC_COUNTS] is overwritten with this call's
 * counters. */
int dbgsom_ctx_sparse_code(dbgsom_ctx *ctx, const void *Xq_host, int x_dtype, int64_t Nq, int64_t d,
                           const double *W_host, int64_t M, int max_iter, const double *P_host,
                           int64_t C, double *code_host, double *proba_host, uint64_t *counts_host);
/* The same on rows in HBM (ldx >= d elements apart, any alignment of the element type): every chunk of
 * "sc_chunk_rows" rows is coded where it lies and written to code_dev + r0 * M / proba_dev + r0 * C (Nq x M / Nq x C
 * float64 device arrays, contiguous) without a staging buffer; W_host, P_host and counts_host are host arrays as above.
 * Blocking; no pointer is retained. */
int dbgsom_ctx_sparse_code_device(dbgsom_ctx *ctx, const void *Xq_dev, int x_dtype, int64_t Nq, int64_t d,
                                  int64_t ldx, const double *W_host, int64_t M, int max_iter,
                                  const double *P_host, int64_t C, double *code_dev, double *proba_dev,
                                  uint64_t *counts_host);

/* ---- topographic function: BaseSom.topographic_function / BaseSom.phi (BaseSom.py:955-998) ------------
 * The graph of the map's induced Delaunay triangulation (an edge {a, b} for every row (a, b) of the
 * samples' first and second BMUs), the hop distance D on it, and the two integer histograms that
 * phi(k) is made of (csrc/topofn.hip):
 *   hist_pos[c], c < n_pos   ordered Delaunay edges (i, j) by the Chebyshev distance c of their lattice
 *                            coordinates; n_pos = max(range of x, range of y) + 1
 *   hist_neg[t], t <= M      ordered lattice 4-neighbour pairs (|dx| + |dy| == 1) by their hop distance
 *                            t (1 .. M - 1); hist_neg[M]: the pairs with no path between them
 *   D (may be NULL)          M x M int32 hop distances, -1 = unreachable (full mode; NULL: histogram
 *                            mode, which stops every source's search once its lattice neighbours have
 *                            their distances -- the histograms are the same)
 * idx2: n x 2 int64 BMU pairs (device); xy: M x 2 int32 lattice coordinates (device), no two alike.
 * M <= DBGSOM_MAX_PROTOTYPES.  ws: dbgsom_topofn_workspace_bytes(M, full) bytes on the device, 256-byte
 * aligned (a misaligned one is DBGSOM_EINVAL, a short one DBGSOM_ENOMEM; both before any launch); its
 * contents on entry do not matter, and nothing outside [ws, ws + ws_bytes) is written.  The call is blocking (it reads back the kernels' status word):
 * DBGSOM_ERANGE when an index is outside [0, M), DBGSOM_EINVAL when an edge spans >= n_pos or two
 * neurons share coordinates. */
size_t dbgsom_topofn_workspace_bytes(int64_t M, int full);
int dbgsom_topofn(const int64_t *idx2_dev, int64_t n, const int32_t *xy_dev, int64_t M, int64_t n_pos,
                  uint64_t *hist_pos_dev, uint64_t *hist_neg_dev, int32_t *D_dev, void *ws,
                  size_t ws_bytes, void *stream);
/* diagnostics: per-stage HIP-event timing of dbgsom_topofn / dbgsom_ctx_topographic_function (calls
 * become blocking while it is on); enabling or disabling resets the sums.  ms4 = summed ms of
 * [k = 2 search (context call only), edge set + CSR + lattice neighbours, distances, histograms] */
int dbgsom_topofn_timing(int enable);
int dbgsom_topofn_stage_ms(double *ms4);
/* The same from host arrays: the k = 2 search of dbgsom_ctx_bmu_query on Xq (Nq x d, DBGSOM_F32 or
 * DBGSOM_F64) against W_host (M x d float64), its pairs kept in HBM, then dbgsom_topofn.
 * hist_pos_host[n_pos], hist_neg_host[M + 1]; D_host (M x M) or NULL. */
int dbgsom_ctx_topographic_function(dbgsom_ctx *ctx, const void *Xq_host, int x_dtype, int64_t Nq,
                                    int64_t d, const double *W_host, int64_t M, int round_f32,
                                    const int32_t *xy_host, int64_t n_pos, int64_t *hist_pos_host,
                                    int64_t *hist_neg_host, int32_t *D_host);
/* The same with the query rows in HBM (placed as dbgsom_ctx_bmu_query_device places them); the histograms and D
 * are host arrays as above. */
int dbgsom_ctx_topographic_function_device(dbgsom_ctx *ctx, const void *Xq_dev, int x_dtype, int64_t Nq,
                                           int64_t d, int64_t ldx, const double *W_host, int64_t M,
                                           int round_f32, const int32_t *xy_host, int64_t n_pos,
                                           int64_t *hist_pos_host, int64_t *hist_neg_host, int32_t *D_host);

/* _calculate_exp_similarity on host values (BaseSom.py:533-538) */
int dbgsom_ctx_exp_similarity(dbgsom_ctx *ctx, const double *dist_host, int64_t n, double gamma,
                              double *kw_host);

/* One pass of the body of BaseSom._grow_som (BaseSom.py:403-407):
 * BMU -> sample kernel -> weighted sums -> [all-reduce] -> smoothing -> convergence norm ->
 * per-neuron error.
 *   W_host     M x d prototypes to start from, or NULL = the resident ones
 *   W_new_host M x d, or NULL: the new prototypes only stay in HBM (they become the resident ones
 *              unless DBGSOM_EPOCH_FROZEN is set)
 * Outputs (host): change_total[1], errors[M], activations[M]; idx_host / dist_host (N each) may be
 * NULL when the caller does not need the assignments. */
int dbgsom_ctx_epoch(dbgsom_ctx *ctx, const double *W_host, int64_t M, int round_f32,
                     double gamma, double sigma, int layout, int flags, double *W_new_host,
                     double *change_total_host, double *errors_host, double *activations_host,
                     int64_t *idx_host, double *dist_host);

/* _update_weights + _write_accumulative_error with the caller's own winners / sample weights /
 * distances (N each, host): BaseSom.py:470-523, 541-561. */
int dbgsom_ctx_update(dbgsom_ctx *ctx, const double *W_host, int64_t M, const int64_t *idx_host,
                      const double *kw_host, const double *dist_host, double sigma, int layout,
                      double *W_new_host, double *change_total_host, double *errors_host,
                      double *activations_host);

/* Seeds of the next filtered search: N winners (any indices < M keep the result exact). */
int dbgsom_ctx_set_hint(dbgsom_ctx *ctx, const int64_t *idx_host, int64_t M);

/* the last epoch's reduced sums [S (M x d) | K | a | E] (diagnostics / tests) */
int dbgsom_ctx_read_sums(dbgsom_ctx *ctx, double *sums_host, int64_t M);

/* ---- reductions around the path on the resident samples (SURVEY 8 f-1 .. f-3) ------------------- */
/* dbgsom_column_sums on the resident samples: out / mean hold d elements of X's dtype */
int dbgsom_ctx_column_sums(dbgsom_ctx *ctx, const void *mean_host, void *out_host);
/* out2 = [sum of BMU distances, number of samples] over all ranks (BaseSom.py:904-922) */
int dbgsom_ctx_quantization_error(dbgsom_ctx *ctx, const double *W_host, int64_t M, int round_f32,
                                  double *out2_host);
/* samples whose two BMUs are further than 1.5 apart on the lattice, over all ranks
 * (BaseSom.py:924-953); xy: M x 2 int32 */
int dbgsom_ctx_topographic_count(dbgsom_ctx *ctx, const double *W_host, int64_t M, int round_f32,
                                 const int32_t *xy_host, double *count_host);
/* hit counts and density sums per neuron over all ranks (BaseSom.py:181-211) */
int dbgsom_ctx_node_statistics(dbgsom_ctx *ctx, const double *W_host, int64_t M, int round_f32,
                               double sigma, double *hits_host, double *density_host);
/* hist[j, c] over all ranks; idx_host = NULL: the winners of the last epoch (still in HBM) */
int dbgsom_ctx_class_histogram(dbgsom_ctx *ctx, const int64_t *idx_host, int64_t n_classes,
                               int64_t M, int64_t *hist_host);

/* ---- per-unit sums of a per-row quantity: a target or an external variable on the map (csrc/unit_sums.hip) ---- */
/* unit: N int64; Z: N x n_values float64, rows ldz >= n_values apart, 1 <= n_values <= DBGSOM_MAX_MIXTURE_VALUES (the
 * result is a legal Y of dbgsom_mixture); w: N float64 weights or NULL; 1 <= M <= DBGSOM_MAX_PROTOTYPES.
 * The list L_j of unit j holds the rows i with unit[i] == j, ascending in i, without the rows with w_i == 0 (a NaN
 * stored under weight 0 is never read).  A row's term is z_iv, or w_i * z_iv rounded once and never fused; its mass
 * term 1.0 or w_i.  L_j is cut into blocks of 128 consecutive list positions, and
 *   P[b][v]    = (((+0.0 + t_0) + t_1) + ...)            the terms of block b in list order, every add rounded
 *   sums[j][v] = (((+0.0 + P[0][v]) + P[1][v]) + ...)    the blocks of unit j ascending;  mass[j] likewise
 * An empty list gives +0.0 bitwise.  Rows whose unit lies outside [0, M) (the -1 of a search that found nothing) are
 * skipped, never followed.  NaN and infinities are plain IEEE: they reach their own (unit, column) only.  The order
 * depends on (unit, Z, w) alone; all weights 1.0 give the bits of no weights.
 *
 * None of these calls takes a stream: each runs on the context's stream and waits for it.  Argument errors -- a null
 * pointer, M or n_values out of range, a row stride below n_values, N < 0 or N >= 2^31, a bad mode -- are DBGSOM_EINVAL
 * before any launch.  N == 0 writes +0.0 sums and masses and launches nothing else.
 *
 * dbgsom_ctx_unit_sums: host arrays; unit, Z (contiguous) and w go up ("x_upload_bytes"), mass (M) and sums (M x
 * n_values, contiguous) come down ("x_download_bytes").  No resident rows are needed.
 * dbgsom_ctx_unit_sums_device: everything in HBM, nothing crosses PCIe; sums rows lds >= n_values apart; nothing of a
 * row of Z or of sums past n_values is touched.
 * dbgsom_ctx_unit_deviations_device: for row i with unit j inside [0, M) and centres C (M x n_values, rows ldc apart),
 * mode DBGSOM_DEVIATIONS_SQUARES writes (y_iv - C_jv)^2 to out (N x n_values, rows ldo apart), mode
 * DBGSOM_DEVIATIONS_NORM writes sqrt(sum_v (y_iv - C_jv)^2) to out (N values; ldo is not read): the sum over v
 * ascending from +0.0, difference, square and add each rounded, the root correctly rounded.  Rows outside [0, M) get
 * +0.0. */
#define DBGSOM_DEVIATIONS_SQUARES 0
#define DBGSOM_DEVIATIONS_NORM 1
int dbgsom_ctx_unit_sums(dbgsom_ctx *ctx, const int64_t *unit_host, const double *Z_host, const double *w_host, int64_t N,
                         int64_t M, int n_values, double *mass_host, double *sums_host);
int dbgsom_ctx_unit_sums_device(dbgsom_ctx *ctx, const int64_t *unit_dev, const double *Z_dev, int64_t ldz,
                                const double *w_dev, int64_t N, int64_t M, int n_values, double *mass_dev,
                                double *sums_dev, int64_t lds);
int dbgsom_ctx_unit_deviations_device(dbgsom_ctx *ctx, const int64_t *unit_dev, const double *Y_dev, int64_t ldy,
                                      int64_t N, const double *C_dev, int64_t ldc, int64_t M, int n_values, int mode,
                                      double *out_dev, int64_t ldo);
/* Targets of the resident rows: N x n_values float64 (host: contiguous; device: rows ldy apart) copied next to the
 * rows; the copy belongs to the context.  N must be the resident N.  (NULL, 0, 0) detaches; a reload detaches too. */
int dbgsom_ctx_set_targets(dbgsom_ctx *ctx, const double *Y_host, int64_t N, int n_values);
int dbgsom_ctx_set_targets_device(dbgsom_ctx *ctx, const double *Y_dev, int64_t N, int64_t ldy, int n_values);
/* Per-unit statistics of the attached targets.  The winners are idx_host (N int64), or with NULL those the last epoch
 * left in HBM (DBGSOM_ESTATE without them, as dbgsom_ctx_class_histogram); the weights are the attached sample weights,
 * if any.  mass (M), mean (M x n_values) = sums / mass, one division, NaN for an empty unit; std (may be NULL)
 * std_jv = sqrt(fold(SQUARES)_jv / mass_j); err (M, may be NULL) err_j = fold(NORM)_j: the weighted sum over the
 * unit's rows of ||y_i - mean_j||_2.  DBGSOM_ESTATE without targets; more than one rank: DBGSOM_EINVAL. */
int dbgsom_ctx_target_statistics(dbgsom_ctx *ctx, const int64_t *idx_host, int64_t M, double *mass_host,
                                 double *mean_host, double *std_host, double *err_host);

/* ---- covariance times a block of directions: the pass of the linear initialisation (covariance.hip) ---- */
#define DBGSOM_MAX_DIRECTIONS 8
/* With c_ik = x_ik - mean_k (x widened to float64, the difference rounded once):
 *   Z[l, j] = sum_i c_il y_ij,  y_ij = sum_k c_ik V[k, j];   colsum[l] = sum_i c_il
 * X: N x d, DBGSOM_F32 or DBGSOM_F64, rows ldx >= d elements apart; no alignment is asked of X or ldx, and the
 * elements between d and ldx of a row are never read.  mean: d float64 (NULL: zeros).  V, Z: d x p row-major float64,
 * 1 <= p <= DBGSOM_MAX_DIRECTIONS; colsum: d float64.  d <= 2^30.  Float64 throughout, no atomics: the result is the
 * same bits for the same (N, d, p) and values, whatever ldx, the alignment of the base, or the run.  A NaN or an
 * infinity in a row goes into Z.  Argument errors are DBGSOM_EINVAL, a short workspace DBGSOM_ENOMEM, both before any
 * launch; N == 0 gives zeros.  Workspace: 16-byte aligned, contents on entry irrelevant, nothing outside
 * [workspace_dev, workspace_dev + workspace_bytes) is written. */
size_t dbgsom_covariance_apply_workspace_bytes(int64_t N, int64_t d, int p);
int dbgsom_covariance_apply(const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx, const double *mean_dev,
                            const double *V_dev, int p, double *Z_dev, double *colsum_dev, void *workspace_dev,
                            size_t workspace_bytes, void *stream);
/* The same on the resident rows; mean (may be NULL), V, Z and colsum are host arrays.  Dense float32 / float64
 * residents only: CSR residents, bfloat16 storage, rows with missing entries, attached sample weights and more than
 * one rank are DBGSOM_EINVAL.  2 d p + 2 d doubles cross PCIe per call ("x_upload_bytes" / "x_download_bytes"),
 * nothing of size N. */
int dbgsom_ctx_covariance_apply(dbgsom_ctx *ctx, const double *mean_host, const double *V_host, int p, double *Z_host,
                                double *colsum_host);

/* ---- vertical growth on Voronoi subsets (BaseSom.py:157-179) ------------------------------------ */
/* BMU of every resident sample under W (NULL = resident prototypes) + stable bucket order;
 * counts_host[M] = samples per neuron on this rank; idx_host (N, may be NULL) = the winners. */
int dbgsom_ctx_partition(dbgsom_ctx *ctx, const double *W_host, int64_t M, int round_f32,
                         int64_t *counts_host, int64_t *idx_host);
/* a new context whose resident samples are the rows of neuron j's Voronoi set (sample order kept),
 * gathered on the device; labels follow when the parent has them */
int dbgsom_ctx_subset_create(dbgsom_ctx *ctx, int64_t neuron, dbgsom_ctx **child);
/* the bucket order dbgsom_ctx_partition left on the device, for tests: order_host[N] int32, the resident rows grouped
 * by unit, ascending inside a unit; seg_start_host[M + 1] uint32, unit j's rows are order[seg_start[j] ..
 * seg_start[j + 1]).  Either may be NULL.  DBGSOM_ESTATE without a valid partition. */
int dbgsom_ctx_read_partition(dbgsom_ctx *ctx, int32_t *order_host, uint32_t *seg_start_host);

/* ---- the nearest stored rows of a query, through the map (csrc/row_neighbors.hip) -------------------- */
/* An inverted-file search: the rows X are filed under units (order / seg_start as above, any order inside a unit), a
 * query q names n_probe units, and its candidates are the rows filed under them.  rho(i, q) is the direct-form squared
 * distance in float64, float32 values widened exactly, in a fixed order: partial l (0 .. 63) takes the features
 * k = l, l + 64, ... ascending, t = x_k - q_k, p_l = p_l + t * t, the difference, the product and the sum each rounded
 * on its own; then six rounds p_l = p_l + p_(l ^ s), s = 32, 16, 8, 4, 2, 1.  Row q of the result holds the k
 * candidates with the smallest (rho, i) in lexicographic order, ascending: idx the row numbers (int64), dist =
 * sqrt(rho) taken after the selection.  Only rho < +inf is listed (never NaN, never an overflow); slots left unfilled
 * hold (inf, -1).  (rho, i) is a total order: the result does not depend on the order inside a unit.
 *
 * dbgsom_ctx_scan_cells_device: the kernel on the caller's device buffers, on the context's stream, waited for.  X: N
 * rows of d features, ldx >= d apart, x_dtype DBGSOM_F32 / DBGSOM_F64; Q likewise (q_dtype, Nq, ldq), the two dtypes
 * independent; bases aligned to their item size.  probe_dev: Nq x n_probe int64, distinct units of a row; an entry
 * outside [0, M) (-1) is skipped.  1 <= n_probe <= min(M, DBGSOM_MAX_NEIGHBORS), 1 <= k <= DBGSOM_MAX_NEIGHBORS,
 * 1 <= d <= DBGSOM_MAX_SCAN_FEATURES (the widened query lives in 64 KiB of LDS); idx_dev / dist_dev: Nq x k.  Entries of
 * order outside [0, N) and segment bounds above N are skipped, never followed.  Argument errors are DBGSOM_EINVAL
 * before any launch; Nq == 0 does nothing.
 *
 * dbgsom_ctx_row_neighbors_query[_device]: the k-nearest-units search of the query (dbgsom_ctx_kneighbors_query: its
 * n_probe indices are the probe list), then the scan over the resident rows and the partition dbgsom_ctx_partition
 * left.  Host rows go up in chunks of "distances_chunk_rows" rows and Nq x k x 16 bytes come down; rows in HBM are
 * read where they are and the kernels write the caller's device arrays.  DBGSOM_ESTATE: no valid partition (none yet,
 * or the samples were loaded again since), M is not the partition's, CSR residents, bfloat16 storage.  d must be the
 * resident rows'. */
#define DBGSOM_MAX_SCAN_FEATURES 8192
int dbgsom_ctx_scan_cells_device(dbgsom_ctx *ctx, const void *X_dev, int x_dtype, int64_t N, int64_t d, int64_t ldx,
                                 const int32_t *order_dev, const uint32_t *seg_start_dev, int64_t M, const void *Q_dev,
                                 int q_dtype, int64_t Nq, int64_t ldq, const int64_t *probe_dev, int n_probe, int k,
                                 int64_t *idx_dev, double *dist_dev);
int dbgsom_ctx_row_neighbors_query(dbgsom_ctx *ctx, const void *Q_host, int q_dtype, int64_t Nq, int64_t d,
                                   const double *W_host, int64_t M, int n_probe, int k, int64_t *idx_host,
                                   double *dist_host);
int dbgsom_ctx_row_neighbors_query_device(dbgsom_ctx *ctx, const void *Q_dev, int q_dtype, int64_t Nq, int64_t d,
                                          int64_t ldq, const double *W_host, int64_t M, int n_probe, int k,
                                          int64_t *idx_dev, double *dist_dev);

/* ---- diagnostics ----------------------------------------------------------------------------- */
/* info8 = [filtered search ran (0/1), mean candidate-list length, digit planes used (0 = no sweep:
 *          triangle pruning), seeds were previous winners (0/1), back-off epochs left, plane-policy
 *          hold, mean list length a counting-only pruning launch found beside the sweep (NaN: none
 *          ran), stateless seeds came from the full pre-pass (0/1)] of the last epoch */
int dbgsom_ctx_epoch_info(dbgsom_ctx *ctx, double *info8);
/* what the engine's search policy has measured: ms12[4 * seeds + planes] = wall clock (ms) of the epoch call
 * when that arm last ran with nothing riding along (seeds 0 = cheap pre-pass, 1 = full pre-pass, 2 = previous
 * winners; planes 0 = triangle pruning, 1 .. 3 = digit planes of the sweep; NaN: not timed / aged out).  Two
 * timed arms are compared by these, the cost model prices the others (engine.hip: adapt_arms). */
int dbgsom_ctx_arm_ms(dbgsom_ctx *ctx, double *ms12);
/* candidate-list length per 128-sample workgroup of the last filtered search (n = ceil(N/128)) */
int dbgsom_ctx_filter_counts(dbgsom_ctx *ctx, uint32_t *counts_host, int64_t n);
/* diagnostics: the anchor buckets of the resident samples ("anchor_state" 1, else DBGSOM_ESTATE); every array may be
 * NULL.  n_anchors: A = min(256, rows); anchors_host: A x padded features float64 (the anchor rows in chain order);
 * anchor_of_host, order_host: one int32 per resident row; aseed_host: A int32, the prototype the last search chose
 * for every anchor -- DBGSOM_ESTATE unless that search was seeded from the anchors. */
int dbgsom_ctx_read_anchors(dbgsom_ctx *ctx, int64_t *n_anchors, double *anchors_host, int32_t *anchor_of_host,
                            int32_t *order_host, int32_t *aseed_host);
/* diagnostics: the run table of those buckets (dbgsom_anchor_runs_read of the context's table; "anchor_state" 1, else
 * DBGSOM_ESTATE).  n_groups: ceil(rows / 128); run_start_host: n_groups + 1 int32 (NULL: only n_groups); the other
 * arrays hold n_groups + n_anchors entries at the most and may be NULL. */
int dbgsom_ctx_read_anchor_runs(dbgsom_ctx *ctx, int64_t *n_groups, int32_t *run_start_host, int32_t *run_anchor_host,
                                double *run_R_host, double *run_xx_host);
/* dbgsom_bmu_filtered_refine_counts of the context's last filtered search */
int dbgsom_ctx_refine_counts(dbgsom_ctx *ctx, uint64_t *out4);
/* ms8 = [bmu, accumulate, smooth, slice W + tables, seed pre-pass, bucket sort, candidate sweep,
 *        exact search on candidates] of the last epoch (option "timing" = 1) */
int dbgsom_ctx_phase_ms(dbgsom_ctx *ctx, double *ms8);

#ifdef __cplusplus
}
#endif
#endif /* DBGSOM_HIP_H */
