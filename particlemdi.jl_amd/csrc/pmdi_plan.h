// pmdi_plan.h -- how every sweep of a handle will be launched, decided once by pmdi_create: a pure function of the configuration,
// the tuning knobs and three facts about the device.  Host-only (no .hip file includes it), no device and no handle: pmdi_plan.cpp
// compiles with any C++ compiler, and tests/plan_main.cpp runs it without a GPU.
#pragma once
#include "pmdi_internal.h"
#include "../../include/pmdi_hip.h"

#include <functional>

// sets the text of pmdi_last_error and returns `code` (pmdi_api.cpp; a stand-alone program brings its own)
int pmdi_set_error(int code, const char *fmt, ...);

// the general kernel's LDS layout at one workgroup width: doubles of the term buffer, and which per-particle tables -- class ids,
// step scratch, column indices -- live in LDS (1) or in global memory (0)
struct LdsTables {
    int terms_cap = 0, pid_lds = 0, pp_lds = 0, col_lds = 0;
};
inline void pmdi_put_tables(const LdsTables &t, SweepArgs &a)
{
    a.terms_cap = t.terms_cap; a.pid_lds = t.pid_lds; a.pp_lds = t.pp_lds; a.col_lds = t.col_lds;
}

struct SweepPlan {
    int T = 0;                   // workgroup width of the general kernel (the heavy group's, when the chains are split)
    int two_per_cu = 0;          // 1: the register-capped build, so that two chains co-reside on a CU
    int ksplit = 0;              // 1: one workgroup per (chain, dataset), meeting once per swept observation
    int ksplit_batch = 0;        // ... chain slots per launch when n_chains * K workgroups are not resident at once (0 = one launch)
    // light group (block_threads == 0 only): chains whose last sweep met few live clusters per step are swept by 256-thread
    // workgroups on a second stream, concurrently with the wide workgroups of the rest
    bool split = false;
    LdsTables wide, light;
    LdsTables resume;            // the general kernel's layout at the settled-chain kernel's workgroup width (hand-over in place)
    long long light_ids = 0;     // a chain is light when its last sweep met at most this many live clusters per step
    // settled-chain kernel (pmdi_sweep2.hip): takes the light group of a sweep when the configuration is one it is built for
    bool s2_ok = false;
    S2Layout s2{};               // its LDS tables after the budget loop (travels in every argument block, used or not)
    bool s2_continue = true;     // a chain that kernel gives back is carried on by the general kernel at that observation
                                 // (false: swept again from the start -- the round-3 behaviour, kept for A/B runs)
    bool requeue_ksplit = true;  // ... swept again by K workgroups when the model has several datasets
    int sticky = 3;              // sweeps a chain stays with the general kernel after the settled-chain kernel gave it back
    int very_heavy = 0;          // the first `very_heavy` heavy chains of the launch order get a CU each (256-register build)
    bool want_gate = false;      // the other launches wait until the heaviest chains' workgroups are placed (needs signal memory)
    bool want_xchg = false;      // the hand-off buffers of the split form (xcnt, xinc, xlab, xhdr) are needed
    bool phase_on = false;
};

// what the plan needs to know about the device
struct PlanDevice {
    int cus = 0;                 // compute units
    bool wait_value = false;     // hipStreamWaitValue32 is usable
    // workgroups per CU of the general kernel's build for this argument block and width; asked only where the split form is
    // tentatively on (anything below 1 counts as 1)
    std::function<int(const SweepArgs &, int T)> blocks_per_cu;
};

// PMDI_OK, or PMDI_E_ARG with the error text set.  Dmax: the widest dataset; cap: cluster ids per dataset
int pmdi_plan_sweep(const pmdi_config &cfg, const pmdi_tuning &tn, int Dmax, long long cap, const PlanDevice &dev, SweepPlan *plan);

// the 32 words of pmdi_sweep_layout (include/pmdi_hip.h); gate / xcnt_allocated: the memory the plan asked for exists
void pmdi_plan_layout32(const SweepPlan &p, bool gate_allocated, bool xcnt_allocated, int K, int P, int32_t out32[32]);
