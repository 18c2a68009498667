// When an epoch's anchor-seeded search may take the lean form (DBGSOM_ANCHOR_LISTS_ONLY, filter_form.h): the lists
// written from the anchors' bounds are final and nothing is made for a per-sample pass behind them.  That is a guess
// that no list will come out long, and the only evidence is the last anchor-seeded epoch: it ran on the same resident
// samples (their anchor buckets have not been rebuilt or dropped since), the same number of prototypes and the same
// plan, it handed no workgroup to the per-sample pass and that pass left no long list.  A wrong guess costs time,
// never the result: the long lists are kept and searched, the epoch reports how many there were, and the next one
// is a full one.  Host-only and free of HIP, like search_policy.h; checked on the CPU by tests/lean_form_check.cpp.
#pragma once

#include <stdint.h>

namespace dbgsom {

struct __attribute__((visibility("hidden"))) LeanGate {
    bool known = false;      // the last epoch was anchor-seeded and its counts came back
    int64_t M = 0;           // prototypes of that epoch
    int64_t generation = 0;  // of the resident samples' anchor buckets (goes up with every load, rebuild and drop)
    int plan = 0;            // the arguments the policy planned for it (seed_stride with its flags, sweep_planes)
    double handed = 0.0, long_lists = 0.0;   // workgroups handed over / lists left long behind the per-sample pass

    static int plan_key(int seed_stride, int sweep_planes) { return seed_stride ^ (sweep_planes << 24); }

    // an epoch that was not anchor-seeded, or whose counts never came back: the next anchor-seeded one is full
    void forget() { known = false; }

    // after an anchor-seeded epoch (lean or full) whose counts came back
    void record(int64_t M_, int64_t generation_, int plan_, double handed_, double long_lists_) {
        known = true; M = M_; generation = generation_; plan = plan_; handed = handed_; long_lists = long_lists_;
    }

    // the anchor-seeded search of the epoch that is about to run: lean?  (retry / refine: what the plan asks for)
    bool allows(int64_t M_, int64_t generation_, int plan_, bool retry, bool refine) const {
        return known && !retry && !refine && M_ == M && generation_ == generation && plan_ == plan && handed == 0.0 &&
               long_lists == 0.0;
    }
};

}  // namespace dbgsom
