// pmdi_host.h -- what the host translation units of the library (the .cpp files) share: error reporting, owned device
// buffers, and the two handle types that more than one of them reads.  Host-only: no .hip file includes it.
#pragma once
#include "pmdi_internal.h"
#include "pmdi_plan.h"
#include "../../include/pmdi_hip.h"

#include <vector>

// pmdi_set_error (declared in pmdi_plan.h; pmdi_api.cpp): sets the text of pmdi_last_error for this thread and returns `code`
constexpr auto fail = pmdi_set_error;       // (the name at the call sites)

#define HIP_TRY(expr)                                                                  \
    do {                                                                               \
        hipError_t e__ = (expr);                                                       \
        if (e__ != hipSuccess)                                                         \
            return fail(e__ == hipErrorOutOfMemory ? PMDI_E_MEMORY : PMDI_E_DEVICE,    \
                        "%s: %s", #expr, hipGetErrorString(e__));                      \
    } while (0)

// device memory an object owns: freed with its owner (which makes its device current before it is deleted)
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int ensure(size_t b)
    {
        if (b <= bytes && p) return 0;
        if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }
        if (b == 0) b = 16;
        hipError_t e = hipMalloc(&p, b);
        if (e != hipSuccess) { p = nullptr; return fail(PMDI_E_MEMORY, "hipMalloc(%zu): %s", b, hipGetErrorString(e)); }
        bytes = b;
        return 0;
    }
};

// device memory of one call, freed on return
struct Scratch {
    void *p = nullptr;
    ~Scratch() { if (p) (void)hipFree(p); }
};

// the launches of a sweep, each with an argument block of its own on the device
enum { ARGS_MAIN = 0, ARGS_LIGHT, ARGS_HEAVIEST, ARGS_SETTLED, ARGS_GIVEN_BACK, ARGS_COUNT };

struct pmdi_handle {
    pmdi_config cfg{};
    pmdi_tuning tun{};           // the creator's knobs (a copy: cfg.tuning is not kept), -1 = automatic
    long long cap = 0;
    int Dmax = 0, sumD = 0, npairs = 1;
    SweepPlan plan;              // how every sweep is launched (pmdi_plan.h), decided once by pmdi_create
    hipStream_t stream = nullptr, stream2 = nullptr, stream3 = nullptr;      // the handle's own; the light launch; the heaviest chains
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_join3 = nullptr;
    unsigned *start_sig = nullptr;   // signal memory: workgroups of the heaviest-chains launch that have started (hipStreamWaitValue32)
    DsetDev ds[PMDI_KMAX_I]{};
    std::vector<void *> owned;          // device allocations freed in destroy
    // per-call staging (device)
    DevBuf d_s_in, d_order, d_Pi, d_logphi, d_flags, d_s_out, d_lw, d_pstar, d_stats, d_err, d_trace;
    DevBuf d_swept_by, d_resume;
    DevBuf d_args[ARGS_COUNT];
    DevBuf d_usc, d_partstar, d_kstate, d_phase, d_requeue, d_requeue_total, d_handed, d_group, d_cost, d_lorder, d_ticket, d_heavy_left, d_stamp, d_work, d_anclog, d_evpos, d_xcnt, d_xinc, d_xlab, d_xhdr;
    bool have_order = false;
    int hold = 0, sweep_grid = 0;       // the settled-chain launch as pmdi_create settled it (pmdi_tuning::hold, sweep_grid; SweepArgs::hold)
    // argument blocks travel through a ring of pinned host slots: the stream-ordered copy is then asynchronous for the host too
    static constexpr int RING = 64;
    SweepArgs *ring = nullptr;
    hipEvent_t ring_ev[RING] = {};
    bool ring_used[RING] = {};
    int ring_head = 0;
    int sweep_no = 0;
    int err_keep = 0;            // set by the device-resident driver around its sweeps (pmdi_gibbs_step)
    int children = 0;            // live pmdi_gibbs / cluster-batch objects: pmdi_destroy refuses while > 0
    // feature selection
    DevBuf d_traj, d_lm, d_firstpos, d_fnull, d_fflags, d_fprob;
    bool swept = false;
    long long last_n1 = 0;
};

// Device-resident Gibbs state of every chain of a handle (pmdi_gibbs_* entry points)
struct pmdi_gibbs {
    pmdi_handle *h = nullptr;
    int device = 0;                      // (cached: destroy must not have to look at the handle)
    GibbsArgs ga{};
    int *s_next = nullptr;               // the sweep's output; exchanged with ga.s after every sweep
    unsigned char *flags = nullptr;      // [chain][sumD] featureFlag
    double *fprob = nullptr;             // [chain][sumD] featureProb of the last feature selection
    double *lw = nullptr;                // [chain][P]
    int *pstar = nullptr;                // [chain]
    long long *stats = nullptr;          // [chain][8]
    int *err = nullptr;                  // [chain]
    long long n1 = 0;
    int feature_select = 0;
    int64_t iter = 0;                    // Gibbs iterations done
    std::vector<void *> owned;
};
