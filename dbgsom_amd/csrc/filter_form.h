// The form of one filtered BMU search: what the flags, the shape and the options of a call resolve to before anything
// is launched -- which seed pre-pass, which candidate kernel, which kernels of the exact stage.  Host-only and free of
// HIP, like search_policy.h: plain arguments in, plain values out, checked on the CPU by tests/filter_form_check.cpp
// (tests/test_filter_form_cpu.py).  launch_bmu_filtered (filter.hip) resolves every call through it -- the engine's and
// dbgsom_bmu_filtered's alike -- and launches what it says.
#pragma once

#include <stdint.h>

#include "../../include/dbgsom_hip.h"

namespace dbgsom {

constexpr int FKT = 64;             // bytes (= features) per plane row per LDS stage: one k-tile
constexpr int PREPASS_KTILES = 3;   // k-tiles the seed pre-pass samples (tile_score_select_kernel picks them)
constexpr int SW_MAX_KT = 1024;     // k-tiles that selection handles (d <= 65536)
constexpr int PRUNE_MAX_M = 8192;   // the gap matrix of the pruning form: 4 M^2 bytes (256 MB here)
constexpr int SWEEP4_MAX_M = 8192;  // bitmask of the two-per-CU sweep's marked prototypes: 1 KB of its LDS

constexpr int64_t FILTER_MAX_D = 0x7fffffc0;   // the kernels take d and filter_dpad(d) as int: the hosts refuse longer rows

// plane rows are padded to whole k-tiles, at least two of them (the sweep's ring runs three tiles
// ahead and keeps three chunk tables)
inline int64_t filter_dpad(int64_t d) {
    // (a 128-byte pitch -- whole cache lines per row -- was measured in round 3: prune_mark_kernel fetched
    //  the same 1.25 GB at d = 784 either way, and the seventh part more plane cost the pre-pass and the
    //  pruning pass 8 % each)
    const int64_t p = (d + FKT - 1) / FKT * FKT;
    return p < 2 * FKT ? 2 * FKT : p;
}

// (hidden: the inline members of a header-only struct must not join the exported symbols of the library)
struct __attribute__((visibility("hidden"))) FilterForm {
    // DBGSOM_SEED_FULL: the seed pre-pass looks at EVERY prototype and every feature (as expensive
    // as the sweep it seeds; what weakly clustered data needs -- the engine's policy decides)
    bool seed_full = false;
    // DBGSOM_PRUNE: candidates from the triangle inequality instead of the sweep (filter.hip 2c);
    // DBGSOM_PRUNE_PROBE: the sweep as usual, and beside it what DBGSOM_PRUNE's lists would add up to
    bool prune = false, prune_probe = false;
    // DBGSOM_PRUNE_RETRY (stateless searches with cheap seeds): workgroups whose pruned lists come out
    // long are re-seeded against every prototype and pruned again (two more short launches)
    bool prune_retry = false;
    bool k2 = false;  // the two nearest prototypes (topographic error, BaseSom.py:945): the pruning form only
    // the seed pre-pass: every seed_stride-th prototype (Msub of them, Msubpad rows of their planes), nkt_used
    // of the row's nkt_full k-tiles (fewer: tile_score_select_kernel picks them)
    int seed_stride = 0, Msub = 0, Msubpad = 0, nkt_full = 0, nkt_used = 0;
    int sweep_planes = 0;  // digit planes per operand, 1 .. 3 (0 resolved to 2)
    // the kernel that writes the candidate lists
    enum Marking {
        MARK_PRUNE,     // prune_mark_kernel alone
        MARK_SWEEP4,    // sweep4_i8_kernel<0>: one product, two workgroups per CU
        MARK_SWEEP_1_4, // sweep_i8_kernel<0, 1, 4>: one product beyond that kernel's bitmask
        MARK_SWEEP_2_2, // sweep_i8_kernel<0, 2, 2>
        MARK_SWEEP_3_1  // sweep_i8_kernel<0, 3, 1>
    } marking = MARK_SWEEP_2_2;
    // MARK_PRUNE on a stateless k = 1 call that brings anchor buckets AND their run table: anchor_mark_kernel writes
    // the lists from the anchors' distances alone (filter.hip 2f), prune_mark_kernel only sees the workgroups whose
    // lists that leaves long.  Everything else -- k = 2, hints, the counting-only probe, anchors without a table --
    // takes prune_mark_kernel over the whole grid.
    bool anchor_mark = false;
    // DBGSOM_ANCHOR_LISTS_ONLY on such a call without the re-seeding and without the refinement: the lean form.
    // anchor_mark_kernel's lists are the lists, long ones included (each is a valid candidate set; the workgroup is
    // only counted as handed over), and nothing that serves the per-sample pass alone is made: no digit planes of
    // W (w_planes), no gap table (gap_nb = 0), no per-sample seeds.  Ignored everywhere else.
    bool lists_only = false;
    bool w_planes = true;   // the call slices W into digit planes (slice_w_tiled_kernel and its tables)
    int gap_nb = 0;  // proto_gap_kernel<gap_nb> (prune, prune_probe): 2 = 64 x 64 tiles, 1 = 32 x 32; 0 = none
    // per-sample refinement (2d): the small tile of its list-length classes, 0 = only the largest
    bool refine = false;
    int rows0 = 0;
    // the matrix-core stage on the candidates
    enum Exact {
        EXACT_K2,             // three launches (one per list-length class) of the k = 2 kernels
        EXACT_BESIDE_REFINE,  // three launches of 64-sample workgroups: what the refinement left
        EXACT_SPLIT,          // one launch, two 64-sample workgroups per bucket: few buckets (nb <= 1024)
        EXACT_ALL             // one launch of all three classes
    } exact = EXACT_ALL;

    // The passes that write the lists of the pruning form (or count them beside a sweep), in launch order.
    // Which pass reports "long lists" to the policy (the count behind pack_results_kernel's third figure, which turns
    // the re-seeding on): the per-sample pass -- PASS_PRUNE_GRID, or PASS_PRUNE_HANDED behind anchor_mark_kernel --
    // and only where it is the last word on a list (prune_retry off); with prune_retry on it lists the workgroups
    // to re-seed instead, and the figure is their number, as ever.  PASS_ANCHOR_MARK never reports: a workgroup it
    // hands to the per-sample pass is not a long list yet.
    enum Pass {
        PASS_ANCHOR_MARK,     // anchor_mark_kernel: every workgroup, from the anchors' bounds; long lists handed on
        PASS_PRUNE_GRID,      // prune_mark_kernel over every workgroup
        PASS_PRUNE_HANDED,    // prune_mark_kernel over the workgroups PASS_ANCHOR_MARK handed on
        PASS_RESEED,          // sweep4_i8_kernel<1> over the workgroups the per-sample pass listed
        PASS_PRUNE_RESEEDED   // prune_mark_kernel over those, final
    };
    int prune_passes(Pass out[4]) const {
        int n = 0;
        if (lists_only) { out[0] = PASS_ANCHOR_MARK; return 1; }
        if (!gap_nb) return 0;
        if (anchor_mark) out[n++] = PASS_ANCHOR_MARK;
        out[n++] = anchor_mark ? PASS_PRUNE_HANDED : PASS_PRUNE_GRID;
        if (prune_retry) { out[n++] = PASS_RESEED; out[n++] = PASS_PRUNE_RESEEDED; }
        return n;
    }
    static bool reports_long_lists(Pass p) { return p == PASS_PRUNE_GRID || p == PASS_PRUNE_HANDED; }

    // nullptr, or why the call is rejected (nothing of *this is then meaningful).  flags: FilteredCall::seed_stride,
    // the stride with DBGSOM_SEED_FULL / DBGSOM_PRUNE / DBGSOM_PRUNE_PROBE / DBGSOM_PRUNE_RETRY /
    // DBGSOM_ANCHOR_LISTS_ONLY OR-ed in;
    // has_hint: the caller brings previous winners (no seed pre-pass).  The shape itself (N, d, M in range) is
    // the launcher's to check.  has_anchors / has_runs: the call brings anchor buckets / their run table.
    const char *resolve(int flags, int planes, int k, int refine_rows, int64_t N, int64_t d, int64_t M, bool has_hint,
                        bool has_anchors = false, bool has_runs = false) {
        seed_full = (flags & DBGSOM_SEED_FULL) != 0;
        prune = (flags & DBGSOM_PRUNE) != 0 && M <= PRUNE_MAX_M;
        prune_probe = !prune && (flags & DBGSOM_PRUNE_PROBE) != 0 && M <= PRUNE_MAX_M;
        prune_retry = (flags & DBGSOM_PRUNE_RETRY) != 0 && !seed_full && !has_hint;
        k2 = k == 2;
        if (!(k == 1 || k == 2)) return "k must be 1 or 2";
        if (!(!k2 || (prune && refine_rows == 0 && M >= 2)))
            return "k = 2 needs the pruning form (DBGSOM_PRUNE, M <= 8192) without the refinement";
        seed_stride = flags & ~(DBGSOM_PRUNE | DBGSOM_PRUNE_PROBE | DBGSOM_PRUNE_RETRY | DBGSOM_ANCHOR_LISTS_ONLY);
        seed_stride = seed_full ? 1 : seed_stride;
        if (!(seed_stride >= 0 && seed_stride <= 64)) return "seed_stride outside [0, 64]";
        if (!(planes >= 0 && planes <= 3)) return "sweep_planes must be 0 .. 3";
        sweep_planes = planes == 0 ? 2 : planes;
        // the seed pre-pass looks at every `seed_stride`-th prototype (any seed keeps the result exact;
        // a coarser pre-pass is cheaper, its seeds are a little further from the minimum)
        // default (0): the stride that makes the subset ONE 256-prototype chunk of the pre-pass, at
        // least 4 -- list lengths barely depend on it (C3: 58 -> 62 from stride 4 to 8, C4 / C5: none)
        if (seed_stride == 0) {
            seed_stride = (int)((M + 255) / 256);
            seed_stride = seed_stride < 4 ? 4 : (seed_stride > 64 ? 64 : seed_stride);
        }
        while (seed_stride > 1 && (M + seed_stride - 1) / seed_stride < 128) seed_stride >>= 1;
        Msub = (int)((M + seed_stride - 1) / seed_stride);
        Msubpad = (Msub + 255) / 256 * 256;
        // ... and at PREPASS_KTILES k-tiles (64 features each) spread evenly over the row, with the
        // matching partial |w|^2: on every workload measured the candidate lists are as short as with
        // all features, the pre-pass costs 0.35 ms at C4 instead of 0.75 with all features
        nkt_full = (int)filter_dpad(d) / FKT;
        nkt_used = (!seed_full && PREPASS_KTILES < nkt_full && nkt_full <= SW_MAX_KT) ? PREPASS_KTILES : nkt_full;
        // The one-product sweep is always the two-per-CU shape (sweep4_i8_kernel, 128 x 256 tile) where its
        // bitmask holds the map, rather than sweep_i8_kernel<0, 1, 4> (128 x 512, one workgroup per CU).
        // Measured on the four BASELINE shapes (ms per launch, one / two per CU): C4 1.37 / 1.11, C3 1.12 /
        // 0.88, C5 shard 4.99 / 4.83, C2 0.059 / 0.058 -- the small shape everywhere, although it reads the
        // X plane once per 256 prototypes instead of once per 512 (C5: 16.4 GB per launch, 3.4 TB/s).
        if (prune) marking = MARK_PRUNE;
        else if (sweep_planes == 1) marking = M <= SWEEP4_MAX_M ? MARK_SWEEP4 : MARK_SWEEP_1_4;
        else marking = sweep_planes == 3 ? MARK_SWEEP_3_1 : MARK_SWEEP_2_2;
        anchor_mark = prune && has_anchors && has_runs && k == 1 && !has_hint && !seed_full;
        // (gaps: 64 x 64 tiles where there are four per CU and more, M >= 2048)
        const int64_t gt = ((M + 63) / 64 * 64) / 64;
        gap_nb = (prune || prune_probe) ? (gt * gt >= 1024 ? 2 : 1) : 0;
        refine = refine_rows > 0;
        // (the re-seeding pass and refine_i8_kernel read the planes of W: no lean form beside either)
        lists_only = (flags & DBGSOM_ANCHOR_LISTS_ONLY) != 0 && anchor_mark && !prune_retry && !refine && k == 1;
        w_planes = !lists_only;
        if (lists_only) gap_nb = 0;
        rows0 = refine_rows <= 32 ? 32 : (refine_rows <= 64 ? 64 : (refine_rows <= 128 ? 128 : 0));
        const int64_t nb = (N + 127) / 128;
        exact = k2 ? EXACT_K2 : (refine ? EXACT_BESIDE_REFINE : (nb <= 1024 ? EXACT_SPLIT : EXACT_ALL));
        return nullptr;
    }
};

}  // namespace dbgsom
