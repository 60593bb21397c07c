// pmdi_plan.cpp -- the launch plan of a handle's sweeps (pmdi_plan.h): pmdi_plan_sweep is a short sequence of steps, each a function
// of its parameters.  No HIP call, no handle: tests/plan_main.cpp runs it on the CPU (tests/test_plan_host.py replays the plans
// recorded on the device through it).
#include "pmdi_plan.h"
#include "pmdi_sweep2_layout.h"
#include "pmdi_sweep_carve.h"

#include <cstring>

namespace {

int knob(int32_t v, int dflt) { return v >= 0 ? (int)v : dflt; }      // (-1 = automatic)

// what every step reads
struct In {
    const pmdi_config &cfg;
    const pmdi_tuning &tn;
    int Dmax;
    long long cap;
};

// the fields of an argument block that size the general kernel's LDS and select its build
SweepArgs sizing_args(const In &in, int ksplit, int two_per_cu, const LdsTables &t)
{
    SweepArgs a;
    memset(&a, 0, sizeof(a));
    a.K = in.cfg.K; a.N = in.cfg.N; a.P = in.cfg.P; a.cap = (int)in.cap; a.Dmax = in.Dmax;
    a.q1 = in.cfg.q1_mode; a.q2 = in.cfg.q2_mode;
    a.item_cap = in.cfg.N > 32 ? PMDI_ITEM_CAP_BIGN : PMDI_ITEM_CAP;
    a.ksplit = ksplit; a.two_per_cu = two_per_cu;
    pmdi_put_tables(t, a);
    return a;
}

bool settled_kernel_possible(const In &in)
{
    return knob(in.tn.settled, 1) != 0 && in.cfg.block_threads == 0 && in.cfg.q1_mode == 0 && in.cfg.q2_mode == 0 &&
           pmdi_sweep2_supports(in.cfg.K, in.cfg.N, in.cfg.P, in.Dmax, in.cap);
}

// K > 1: one workgroup per (chain, dataset), meeting once per swept observation (pmdi_sweep.hip): 2.2x shorter sweeps per
// chain, but the partners repeat the per-observation serial work (weights, ESS, resampling indices), so when the chains alone
// can fill the GPU the single-workgroup form has the higher aggregate throughput.  Default: split while every workgroup of
// the split launch is RESIDENT at once -- checked by `residency_batch`, once the LDS layout and the register-capped / uncapped build are
// known.  ksplit = 0/1 forces either form.  The history-permuting __pmdi mode (q2_mode = 1) always keeps the single-workgroup
// form: its ancestor log is per chain.
// ... unless the handle can have the settled-chain kernel (round 4): ONE workgroup of it sweeps a settled chain faster than the K
// cooperating workgroups of the general kernel do (HL, one chain alone on the GPU: 3.18 against 2.98-3.00 iterations/s,
// bench.py `one_chain_alone`), on a quarter of the workgroup slots
int tentative_split_form(const In &in)
{
    const bool ks_ok = in.cfg.K > 1 && in.cfg.q2_mode == 0 && (long long)in.cfg.K * in.cfg.n < (1LL << 27);
    const bool s2_possible = in.cfg.K >= 2 && settled_kernel_possible(in);
    return (ks_ok && in.tn.ksplit != 0 && !(in.tn.ksplit < 0 && s2_possible)) ? 1 : 0;
}

// per workgroup width: LDS term buffer (at least P doubles for the resampling weights, the
// per-wave CDF exchange areas, a few rows of 2*D+1) and which per-particle tables fit LDS
int lds_tables(const In &in, int T, int ksplit, LdsTables *out)
{
    const int N = in.cfg.N, P = in.cfg.P;
    int tc = knob(in.tn.terms_cap, 1024);
    if (tc < P) tc = P;
    if (tc < (T / 64) * (N > 64 ? 512 : 128)) tc = (T / 64) * (N > 64 ? 512 : 128);   // per-wave exchange areas of the CDF stage
    if (tc < 4 * (2 * in.Dmax + 1)) tc = 4 * (2 * in.Dmax + 1);
    if (tc < 384) tc = 384;                                   // the known-prefix label table (3 x 256 ints) lives there
    LdsTables t;
    t.terms_cap = tc;
    auto bytes = [&](int pid, int pp, int col) {
        t.pid_lds = pid; t.pp_lds = pp; t.col_lds = col;
        return pmdi_sweep_lds_bytes(sizing_args(in, ksplit, 0, t), T);
    };
    // Two chains per CU (<= 80 KiB each) hide each other's dependent latencies: +40 % aggregate throughput on the
    // headline workload even with the per-particle tables in global memory.  So: the largest set of per-particle
    // tables that still fits 80 KiB; if none does, one chain per CU with everything that fits 150 KiB in LDS.
    const bool tgt = in.tn.lds_target >= 0;
    const size_t half = 80 * 1024 - 256;      // half a CU's 160 KiB, less the kernel's static LDS (256 bytes of reduction scratch)
    bool fits_half = false;
    // (what a step reads of them, most often first: the column indices -- every step --, the step scratch, the class ids
    // -- only in steps with more than one particle class)
    for (int opt = 0; opt < 4 && !tgt && !fits_half; ++opt) fits_half = bytes(opt < 1, opt < 3, opt < 2) <= half;
    if (!fits_half) {
        const size_t lds_target = tgt ? (size_t)in.tn.lds_target : (size_t)150 * 1024;
        if (bytes(1, 1, 1) > lds_target) t.pid_lds = 0;                          // class ids of K*P particles do not fit: global memory
        if (bytes(t.pid_lds, 1, 1) > lds_target) t.pp_lds = 0;                   // nor does the per-particle step scratch
        if (bytes(t.pid_lds, t.pp_lds, 1) > lds_target) t.col_lds = 0;           // nor do the column indices
    }
    const size_t total = bytes(t.pid_lds, t.pp_lds, t.col_lds);
    if (total > 160 * 1024) return pmdi_set_error(PMDI_E_ARG, "configuration needs %zu bytes of LDS (> 160 KiB)", total);
    *out = t;
    return PMDI_OK;
}

int wide_layout(const In &in, int T, int ksplit, LdsTables *wide, int *two_per_cu)
{
    const int rc = lds_tables(in, T, ksplit, wide);
    if (rc) return rc;
    *two_per_cu = knob(in.tn.two_per_cu, 1);
    // one chain per CU anyway: the 256-register build (no spills) instead of the register-capped one
    if (in.tn.two_per_cu < 0 && pmdi_sweep_lds_bytes(sizing_args(in, ksplit, 0, *wide), T) > 80 * 1024 - 256) *two_per_cu = 0;
    return PMDI_OK;
}

// Split form: chain slots that are resident together, in whole groups of eight (the slots are dealt in groups of eight); 0 when
// every workgroup of the launch is resident at once.  A chain whose K workgroups straddle the residency limit would spin in its
// hand-off until some other chain's whole sweep has ended.
int residency_batch(const In &in, const PlanDevice &dev, const SweepArgs &a, int T)
{
    int blocks = dev.blocks_per_cu ? dev.blocks_per_cu(a, T) : 1;
    if (blocks < 1) blocks = 1;
    const long long capacity = (long long)blocks * dev.cus;
    const long long grid = ((long long)(in.cfg.n_chains + 7) / 8) * 8 * in.cfg.K;
    if (grid <= capacity) return 0;
    const long long b = capacity / (8LL * in.cfg.K) * 8;
    return (int)(b < 8 ? 8 : b);
}

// the settled-chain kernel: configurations of the shapes it is built for (any mix of the three cluster types), the reference's
// default quirk modes, one workgroup per chain; its LDS tables sized so that two 256-thread chains share a CU (fewer LDS columns /
// ids if need be); a 512-thread chain (P = 2 048) has a CU's registers to itself and may take its LDS too.
// (K = 1: three of its four waves would idle through the cluster phases -- cfg2 runs 2 812 it/s on the general kernel's
// one-dataset build and 2 086 with this kernel; settled = 2 forces it for the tests of its K = 1 instantiations)
bool settled_tables(const In &in, int ksplit, S2Layout *s2)
{
    const int K = in.cfg.K, N = in.cfg.N, P = in.cfg.P;
    if (!((K >= 2 || knob(in.tn.settled, 1) == 2) && !ksplit && settled_kernel_possible(in))) return false;
    const size_t budget = pmdi_sweep2_threads(K, P) > 256 ? (size_t)159 * 1024 : (size_t)80 * 1024;
    int cols_l = knob(in.tn.s2_cols, 64), idcap = knob(in.tn.s2_idcap, 128);
    if (cols_l < 1) cols_l = 1;
    if (cols_l > P) cols_l = P;
    if (idcap < 8) idcap = 8;
    if (idcap > 4096) idcap = 4096;
    // particle classes per dataset the LDS tables hold: as many as the budget allows, 32 at most (a step with more hands the
    // chain over to the general kernel: with N labels a single ambiguous observation fans one class out into up to N)
    int cls = knob(in.tn.s2_cls, 32);
    if (cls < 16) cls = 16;
    if (cls > pmdi_sweep2_max_classes(K, P)) cls = pmdi_sweep2_max_classes(K, P);
    cls &= ~3;
    // (the mutation-CDF rows of the class slots beyond the first 16 go to the chain's arena before the class count shrinks: a
    // step with that many classes is rare, a hand-over costs the rest of the chain's sweep at the general kernel's speed)
    int cdfl = cls;
    auto over = [&]() { pmdi_sweep2_layout(K, N, P, in.Dmax, cols_l, idcap, cls, cdfl, s2); return (size_t)s2->total > budget; };
    bool o = over();
    if (o && cls > 16 && pmdi_sweep2_cdf_arena(K, P)) { cdfl = 16; o = over(); }
    while (o && cls > 16) { cls -= 4; if (cdfl > cls) cdfl = cls; o = over(); }
    while (o && (cols_l > 16 || idcap > 64)) {
        // (a settled chain holds 6-40 columns and ids below ~40 at the 99th percentile of its steps: the id tables go first)
        if (idcap > 96) idcap -= 16; else if (cols_l > 32) cols_l -= 8; else if (idcap > 64) idcap -= 16; else cols_l -= 8;
        o = over();
    }
    return !o;
}

}  // namespace

int pmdi_plan_sweep(const pmdi_config &cfg, const pmdi_tuning &tn, int Dmax, long long cap, const PlanDevice &dev, SweepPlan *plan)
{
    const In in{cfg, tn, Dmax, cap};
    SweepPlan p;
    int rc;
    p.T = cfg.block_threads ? cfg.block_threads : (cfg.P >= 2048 ? 1024 : (cfg.P > 256 ? 512 : 256));
    if (!cfg.block_threads && p.T > 256 && tn.heavy_threads > 0) p.T = tn.heavy_threads;   // tuning knob: width of the heavy group
    if (p.T != 128 && p.T != 256 && p.T != 512 && p.T != 1024) return pmdi_set_error(PMDI_E_ARG, "block_threads must be 128, 256, 512 or 1024");
    // (a step whose particle classes' (class, label) items outgrow the LDS tables takes the general route through global memory;
    // one class always fits: N <= 255 < 384)
    if (cfg.N > (cfg.N > 32 ? PMDI_ITEM_CAP_BIGN : PMDI_ITEM_CAP)) return pmdi_set_error(PMDI_E_ARG, "N=%d too large for the LDS tables", cfg.N);
    p.phase_on = tn.phase_timers > 0;
    p.requeue_ksplit = tn.requeue_ksplit != 0;

    p.ksplit = tentative_split_form(in);
    if ((rc = wide_layout(in, p.T, p.ksplit, &p.wide, &p.two_per_cu))) return rc;
    if (p.ksplit) {
        const int batch = residency_batch(in, dev, sizing_args(in, 1, p.two_per_cu, p.wide), p.T);
        if (batch && tn.ksplit < 0) {            // default: the single-workgroup form (and its own LDS layout)
            p.ksplit = 0;
            if ((rc = wide_layout(in, p.T, 0, &p.wide, &p.two_per_cu))) return rc;
        } else {                                 // forced: residency-sized batches one after the other
            p.ksplit_batch = batch;
        }
    }
    p.s2_ok = settled_tables(in, p.ksplit, &p.s2);

    // automatic width: split the chains of a sweep into a heavy and a light launch
    p.split = cfg.block_threads == 0 && (p.T > 256 || p.s2_ok) && knob(tn.split, 1) != 0;
    if (!p.split) p.s2_ok = false;
    // A chain is "light" when its last sweep met few live clusters per step.  With the settled-chain kernel: as many as that kernel's
    // LDS id tables hold (it evaluates any number in place -- HL's busiest chains, 40-90 ids per step, run 20 % faster there than
    // in the general kernel -- but a K = 1 chain that never resamples keeps thousands of private clusters, and those steps belong to
    // the general kernel's hash tables: cfg2 with every chain light took 3.4 s per sweep instead of 0.8).  Without it: 40.
    p.light_ids = knob(tn.light_ids, p.s2_ok ? p.s2.idcap : 40);
    if (p.s2_ok && knob(tn.settled, 1) == 2) p.light_ids = 1LL << 40;      // (tests: every chain starts every sweep on the settled-chain kernel)
    p.sticky = knob(tn.sticky, 3);
    p.s2_continue = knob(tn.continue_inplace, 1) != 0;
    // a light layout that does not fit turns the heavy / light split off (and the settled-chain kernel with it) ...
    if (p.split && lds_tables(in, 256, p.ksplit, &p.light)) p.split = p.s2_ok = false;
    // ... a hand-over layout that does not fit only the continuation in place
    if (p.split && p.s2_ok) {
        const int thr = pmdi_sweep2_threads(cfg.K, cfg.P);
        if (thr == 256) p.resume = p.light;
        else if (lds_tables(in, thr, p.ksplit, &p.resume)) p.s2_continue = false;
    }
    if (p.split) {
        // (with the settled-chain kernel only the few chains it gave back lately are heavy at all: no CU-each launch for them --
        // HL 1 160 it/s without against 1 146 with it -- and so no start gate either, which a profiler would switch off)
        p.very_heavy = (p.T == 512 && p.two_per_cu) ? knob(tn.very_heavy, p.s2_ok ? 0 : 128) : 0;
        // (not under a profiler that collects counters: rocprofv3 --pmc runs the kernels of all queues one at a time, and a launch
        // that waits for another launch's workgroups then never starts -- observed as a hang of the FETCH_SIZE pass)
        p.want_gate = p.very_heavy > 0 && dev.wait_value && !(tn.profiled > 0) && knob(tn.start_gate, 1) != 0;
    }
    p.want_xchg = p.ksplit || (p.s2_ok && cfg.K > 1 && (long long)cfg.K * cfg.n < (1LL << 27));
    *plan = p;
    return PMDI_OK;
}

void pmdi_plan_layout32(const SweepPlan &p, bool gate_allocated, bool xcnt_allocated, int K, int P, int32_t out32[32])
{
    for (int i = 0; i < 32; ++i) out32[i] = 0;
    const bool handover = p.split && p.s2_ok && p.s2_continue;
    auto group = [&](int at, int threads, const LdsTables &t) {
        const int g[5] = { threads, t.terms_cap, t.pid_lds, t.pp_lds, t.col_lds };
        for (int j = 0; j < 5; ++j) out32[at + j] = threads ? g[j] : 0;
    };
    group(0, p.T, p.wide);
    group(5, p.split ? 256 : 0, p.light);
    group(10, handover ? pmdi_sweep2_threads(K, P) : 0, p.resume);
    out32[15] = p.two_per_cu; out32[16] = p.split ? 1 : 0; out32[17] = p.ksplit; out32[18] = p.ksplit_batch;
    out32[19] = p.split ? p.very_heavy : 0;
    out32[20] = (p.split && p.very_heavy > 0 && gate_allocated && !p.ksplit) ? 1 : 0;
    out32[21] = p.s2_ok ? 1 : 0;
    if (p.s2_ok) {
        out32[22] = p.s2.cols_l; out32[23] = p.s2.idcap; out32[24] = p.s2.cls; out32[25] = p.s2.cdfl;
        out32[26] = pmdi_sweep2_threads(K, P); out32[27] = p.s2.total;
        out32[28] = p.s2_continue ? 1 : 0;
        out32[29] = (!p.s2_continue && K > 1 && xcnt_allocated && p.requeue_ksplit) ? 1 : 0;
    }
}
