// pmdi_api.cpp -- host side of the C ABI declared in include/pmdi_hip.h.
// Converts the reference's conventions (column-major, 1-based Int64) at the
// boundary, owns device memory, builds the exact-arithmetic lookup tables and
// launches the kernels of pmdi_kernels.hip.  No CPU fallback exists: every
// compute entry point runs on the gfx950 device or fails.
#include "pmdi_arith.h"           // uniform01: the initial feature flags
#include "pmdi_host.h"
#include "pmdi_data_groupsum_plan.h"
#include "pmdi_psm_blocksum_plan.h"
#include "pmdi_sweep_carve.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <utility>
#include <vector>

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

namespace {

thread_local char g_err[512] = "";

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// the divisor of the `which` matrix of counts (pmdi_psm_*_device): S, or S K for the Overall one
unsigned __int128 psm_divisor(int64_t S, int32_t K, int32_t which) { return (unsigned __int128)S * (unsigned)(which == K ? K : 1); }

// fills the arena offsets of one dataset; returns the per-chain stride
size_t layout_arena(DsetDev &d, int N, int P, long long cap, long long n_rows_sstar, bool sweep_state)
{
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o = align_up(o + bytes, 256); return at; };
    const size_t ids = (size_t)cap + 1;
    if (sweep_state) {
        d.o_particle[0] = take((size_t)N * P * 4);
        d.o_particle[1] = take((size_t)N * P * 4);
        d.o_col = take((size_t)P * 4);
        d.o_cgrp = take((size_t)(N > 3 ? N : 3) * P * 8);      // (the settled-chain kernel keeps 20 bytes per column there: N = 2 would not hold them)
        d.o_pid = take((size_t)P * 4);
        d.o_sid = take((size_t)P * 4);
        d.o_kv = take((size_t)P * 4);
        d.o_newid = take((size_t)N * P * 4);
        d.o_counts = take(ids * 4);
        d.o_ncop = take(ids * 4);
        d.o_firstc = take(ids * 4);
        d.o_lp = take(ids * 8);
        d.o_sstar = take((size_t)n_rows_sstar * P);
        d.o_clslead = take((size_t)P * 4);
        d.o_clsval = take((size_t)P * 4);
        d.o_cdf = take((size_t)P * (N + 2) * 8);
        d.o_dl = take((size_t)3 * P * 4);
        d.o_s2x = take((size_t)2048 * 12);
    }
    d.o_cn = take(ids * 4);
    if (d.kind == K_GAUSSIAN) {
        if (!sweep_state) d.o_ml = take(ids * d.D * 16);   // stand-alone batches keep (mu, lambda) as stored values
        d.o_sb = take(ids * d.D * 16);
    } else if (d.kind == K_CATEGORICAL) {
        d.o_cnt = take(ids * d.D * d.L * 4);
    } else {
        d.o_nbs = take(ids * d.D * 8);
    }
    return o;
}

}  // namespace

// error reporting of every translation unit of the library (declared in pmdi_host.h)
int pmdi_set_error(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// the conditions the functions that take a `which` matrix of counts share; 0 or PMDI_E_ARG.
// cand: the function takes B candidates ld labels apart and sums over at most PMDI_KMAX datasets; pmdi_psm_distance_device
// (pmdi_hclust.hip) does neither and keeps its own wording of the range
int pmdi_psm_shared_args(const char *who, int64_t S, int32_t K, int64_t n, int32_t which, bool cand, int64_t B, int64_t ld)
{
    if (cand && (K < 1 || K > PMDI_KMAX || S < 1 || n < 1 || n > 65535 || B < 1 || ld < n))
        return fail(PMDI_E_ARG, "%s: S=%lld K=%d n=%lld B=%lld ld=%lld out of range (K <= %d, n <= 65535, ld >= n)", who,
                    (long long)S, K, (long long)n, (long long)B, (long long)ld, PMDI_KMAX);
    if (!cand && (S < 1 || K < 1 || n < 1 || n > 65535))
        return fail(PMDI_E_ARG, "%s: S=%lld K=%d n=%lld out of range (n <= 65535)", who, (long long)S, K, (long long)n);
    if (which < 0 || which > K || (which == K && K == 1))
        return fail(PMDI_E_ARG, "%s: which=%d, but there are %d matrices (the Overall one only for K > 1)", who, which, K + (K > 1));
    return PMDI_OK;
}

struct pmdi_cluster_batch {
    pmdi_handle *h = nullptr;
    int k = 0, B = 0;
    DsetDev d{};
    void *arena = nullptr;
    DevBuf d_rows, d_flags, d_out;
};

namespace {

int dev_alloc(pmdi_handle *h, void **p, size_t bytes)
{
    if (bytes == 0) bytes = 16;
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) { *p = nullptr; return fail(PMDI_E_MEMORY, "hipMalloc(%zu bytes): %s", bytes, hipGetErrorString(e)); }
    h->owned.push_back(*p);
    return 0;
}

template <class Tt>
int upload(pmdi_handle *h, const std::vector<Tt> &v, const Tt **out)
{
    void *p = nullptr;
    int rc = dev_alloc(h, &p, v.size() * sizeof(Tt));
    if (rc) return rc;
    if (!v.empty()) HIP_TRY(hipMemcpy(p, v.data(), v.size() * sizeof(Tt), hipMemcpyHostToDevice));
    *out = (const Tt *)p;
    return 0;
}

void fill_sweep_common(const pmdi_handle *h, SweepArgs &a)
{
    memset(&a, 0, sizeof(a));
    a.K = h->cfg.K; a.N = h->cfg.N; a.P = h->cfg.P; a.cap = (int)h->cap;
    a.Dmax = h->Dmax; a.sumD = h->sumD; a.npairs = h->npairs;
    a.q1 = h->cfg.q1_mode; a.q2 = h->cfg.q2_mode;
    const SweepPlan &pl = h->plan;
    pmdi_put_tables(pl.wide, a);
    a.item_cap = h->cfg.N > 32 ? PMDI_ITEM_CAP_BIGN : PMDI_ITEM_CAP;
    a.two_per_cu = pl.two_per_cu;
    a.phase = pl.phase_on ? (long long *)h->d_phase.p : nullptr;
    a.stamp = pl.phase_on ? (long long *)h->d_stamp.p : nullptr;
    a.cost = (long long *)h->d_cost.p;
    a.work = (long long *)h->d_work.p;
    a.anclog = (int *)h->d_anclog.p; a.evpos = (int *)h->d_evpos.p;
    a.ksplit = pl.ksplit; a.xcnt = (int *)h->d_xcnt.p; a.xinc = (double *)h->d_xinc.p; a.xlab = (int *)h->d_xlab.p; a.xhdr = (unsigned long long *)h->d_xhdr.p;
    a.chain_order = h->have_order ? (const int *)h->d_lorder.p : nullptr;
    a.s2 = pl.s2;
    a.requeue = pl.s2_ok ? (int *)h->d_requeue.p : nullptr;
    a.requeue_total = pl.s2_ok ? (long long *)h->d_requeue_total.p : nullptr;
    a.handed = pl.s2_ok ? (int *)h->d_handed.p : nullptr;
    a.sweep_no = h->sweep_no;
    a.swept_by = (int *)h->d_swept_by.p;
    a.resume = (pl.s2_ok && pl.s2_continue) ? (int *)h->d_resume.p : nullptr;
    a.n = h->cfg.n;
    a.seed = h->cfg.seed;
    for (int k = 0; k < h->cfg.K; ++k) a.ds[k] = h->ds[k];
}

// what a call of pmdi_sweep / pmdi_sweep_device adds to the handle's part of the argument block: its inputs and outputs (device
// pointers; pstar / stats / err null: the handle's own buffers)
void fill_sweep_call(const pmdi_handle *h, SweepArgs &a, int64_t iter, int64_t n1, double lw_init, const int *s_in, const int *order,
                     const double *Pi, const double *logphi, const unsigned char *flags, int *s_out, double *lw_out, int *pstar,
                     long long *stats, int *err, double *trace)
{
    fill_sweep_common(h, a);
    a.iter = (unsigned)iter; a.n1 = n1; a.lw_init = lw_init;
    a.s_in = s_in; a.order = order; a.Pi = Pi; a.logphi = logphi; a.flags = flags;
    a.s_out = s_out; a.lw_out = lw_out;
    a.pstar = pstar ? pstar : (int *)h->d_pstar.p;
    a.stats = stats ? stats : (long long *)h->d_stats.p;
    a.err = err ? err : (int *)h->d_err.p;
    a.trace = trace; a.trace_on = trace ? 1 : 0;
    a.uscratch = (double *)h->d_usc.p; a.partstar = (int *)h->d_partstar.p; a.kstate = (int *)h->d_kstate.p;
}

// next pinned staging slot of the handle's ring (waits -- normally not at all -- for the copy that last used it)
SweepArgs *next_slot(pmdi_handle *h, hipStream_t st_of_copy, int *idx)
{
    (void)st_of_copy;
    if (!h->ring) { *idx = -1; return nullptr; }
    const int i = h->ring_head;
    h->ring_head = (i + 1) % pmdi_handle::RING;
    if (h->ring_used[i]) (void)hipEventSynchronize(h->ring_ev[i]);
    *idx = i;
    return h->ring + i;
}

hipError_t launch_one(pmdi_handle *h, const SweepArgs &a, SweepArgs *d_args, int n_chains, int T, hipStream_t st)
{
    int idx;
    SweepArgs *slot = next_slot(h, st, &idx);
    hipError_t e = pmdi_launch_sweep(a, d_args, n_chains, T, st, slot);
    if (e == hipSuccess && idx >= 0) { e = hipEventRecord(h->ring_ev[idx], st); h->ring_used[idx] = true; }
    return e;
}

// split mode: all chain slots in one launch when their K workgroups each are resident at once, else in residency-sized batches
// one after the other (a chain whose partners straddle the residency limit would spin until some other chain's whole sweep ends)
hipError_t launch_maybe_batched(pmdi_handle *h, const SweepArgs &a, SweepArgs *d_args, int n_chains, int T, hipStream_t st)
{
    const int batch = h->plan.ksplit_batch;
    if (!a.ksplit || batch <= 0 || n_chains <= batch) return launch_one(h, a, d_args, n_chains, T, st);
    for (int b0 = 0; b0 < n_chains; b0 += batch) {
        SweepArgs ab = a;
        ab.n_slots = n_chains; ab.slot_base = b0;
        const int nb = (n_chains - b0 < batch) ? n_chains - b0 : batch;
        hipError_t e = launch_one(h, ab, d_args, nb, T, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// One sweep of all chains on stream `st`: a single launch, or (automatic width) the heavy chains in
// wide workgroups on `st` and the light ones in 256-thread workgroups on the handle's second stream,
// forked from and joined back into `st`.  Then the launch order and groups of the next sweep.
int launch_sweep_groups(pmdi_handle *h, SweepArgs &a, hipStream_t st)
{
    const int C = h->cfg.n_chains;
    const SweepPlan &pl = h->plan;
    auto args = [&](int which) { return (SweepArgs *)h->d_args[which].p; };
    hipError_t e;
    a.err_keep = h->err_keep;
    a.sweep_no = ++h->sweep_no;        // (counts the sweeps of this handle: how long ago was a chain given back?)
    // nobody is on the list of given-back chains when a sweep starts (a chain whose re-run failed must not be swept by two launches
    // of the next sweep at once)
    if (pl.s2_ok) HIP_TRY(hipMemsetAsync(h->d_requeue.p, 0, (size_t)C * 4, st));
    if (pl.ksplit) {       // arrival counters of the hand-offs; the K workgroups of a chain ADD their counters into stats
        HIP_TRY(hipMemsetAsync(h->d_xcnt.p, 0, (size_t)C * 32 * 4, st));
        HIP_TRY(hipMemsetAsync(a.stats, 0, (size_t)C * 64, st));
        if (!h->err_keep) HIP_TRY(hipMemsetAsync(a.err, 0, (size_t)C * 4, st));
    }
    if (!pl.split) {
        e = launch_maybe_batched(h, a, args(ARGS_MAIN), C, pl.T, st);
        if (e != hipSuccess) return fail(PMDI_E_DEVICE, "sweep launch: %s", hipGetErrorString(e));
    } else {
        HIP_TRY(hipEventRecord(h->ev_fork, st));
        a.group_flag = (const unsigned char *)h->d_group.p;
        a.group_sel = 1;
        // the heavy launches count their workgroups in: the settled-chain launch's workgroups keep their slots once all are placed
        a.heavy_left = pl.s2_ok ? (int *)h->d_heavy_left.p : nullptr;
        const int vh = pl.very_heavy < C ? pl.very_heavy : C;
        if (vh > 0) {
            // the heaviest chains bound the launch: they get the 256-register build, one CU each
            SweepArgs av = a;
            av.two_per_cu = 0; av.rank_lo = 0; av.rank_hi = vh;
            HIP_TRY(hipStreamWaitEvent(h->stream3, h->ev_fork, 0));
            // A workgroup of that build needs a CU to itself.  If the other two launches were released at the same moment their
            // smaller workgroups would take a slot on every CU first and the heaviest chains -- the ones that bound the sweep --
            // would start late, one by one, whenever a CU happens to drain (measured at cfg2: 1 020 ms for a launch whose chains
            // take 550 ms).  So its workgroups count themselves in on entry and the other launches wait for that count.
            const bool gate = h->start_sig != nullptr && !pl.ksplit;
            if (gate) av.start_sig = h->start_sig;      // (zero here: reset on `st` behind the previous sweep's join, below)
            e = launch_one(h, av, args(ARGS_HEAVIEST), vh, pl.T, h->stream3);
            if (e != hipSuccess) return fail(PMDI_E_DEVICE, "sweep launch (heaviest chains): %s", hipGetErrorString(e));
            HIP_TRY(hipEventRecord(h->ev_join3, h->stream3));
            if (gate) {
                const unsigned n_wg = (unsigned)vh;
                HIP_TRY(hipStreamWaitValue32(st, h->start_sig, n_wg, hipStreamWaitValueGte, 0xFFFFFFFFu));
                HIP_TRY(hipStreamWaitEvent(h->stream2, h->ev_fork, 0));
                HIP_TRY(hipStreamWaitValue32(h->stream2, h->start_sig, n_wg, hipStreamWaitValueGte, 0xFFFFFFFFu));
            }
        }
        a.rank_lo = vh; a.rank_hi = C;
        e = launch_maybe_batched(h, a, args(ARGS_MAIN), C, pl.T, st);
        if (e != hipSuccess) return fail(PMDI_E_DEVICE, "sweep launch (heavy group): %s", hipGetErrorString(e));
        if (vh > 0) HIP_TRY(hipStreamWaitEvent(st, h->ev_join3, 0));
        SweepArgs al = a;
        al.group_sel = 0; al.rank_lo = 0; al.rank_hi = C;
        al.heavy_left = nullptr;
        pmdi_put_tables(pl.light, al);
        HIP_TRY(hipStreamWaitEvent(h->stream2, h->ev_fork, 0));
        if (pl.s2_ok) {
            // the light chains go to the settled-chain kernel.  A chain whose step does not fit its tables is carried on from that
            // observation by the general kernel's code in the same workgroup: the argument block holds the general kernel's LDS
            // layout for that workgroup width
            pmdi_put_tables(pl.resume, al);
            int idx;
            SweepArgs *slot = next_slot(h, h->stream2, &idx);
            SweepArgs as = al;
            // its workgroups draw their positions in the launch order instead of taking blockIdx.x (SweepArgs::ticket; PMDI_TICKET=0: dealt)
            as.ticket = (h->tun.ticket != 0) ? (int *)h->d_ticket.p : nullptr;
            // ... and, once the heavy chains' workgroups are all placed, keep their slots and draw again until the order is used up:
            // no slot stands idle while chains are left, whatever share of the workgroup indices its dispatch queue was dealt
            as.hold = h->hold;
            as.heavy_left = (int *)h->d_heavy_left.p;
            e = pmdi_launch_sweep2(as, args(ARGS_SETTLED), C, h->sweep_grid, h->stream2, slot);
            if (e == hipSuccess && idx >= 0) { e = hipEventRecord(h->ring_ev[idx], h->stream2); h->ring_used[idx] = true; }
            if (e != hipSuccess) return fail(PMDI_E_DEVICE, "sweep launch (settled chains): %s", hipGetErrorString(e));
            if (!pl.s2_continue) {
                // (PMDI_CONTINUE=0, the round-3 behaviour kept for A/B runs: no hand-over record; the chains that kernel gives back are
                // swept again FROM THE START by the general kernel right behind it -- with one workgroup per dataset when the model has several)
                SweepArgs ar = al;
                ar.group_flag = nullptr; ar.requeue_only = 1;
                pmdi_put_tables(pl.light, ar);
                if (h->cfg.K > 1 && h->d_xcnt.p && pl.requeue_ksplit) {
                    ar.ksplit = 1;
                    HIP_TRY(hipMemsetAsync(h->d_xcnt.p, 0, (size_t)C * 32 * 4, h->stream2));
                }
                e = launch_one(h, ar, args(ARGS_GIVEN_BACK), C, 256, h->stream2);
                if (e != hipSuccess) return fail(PMDI_E_DEVICE, "sweep launch (chains given back by the settled-chain kernel): %s", hipGetErrorString(e));
            }
        } else {
            e = launch_maybe_batched(h, al, args(ARGS_LIGHT), C, 256, h->stream2);
            if (e != hipSuccess) return fail(PMDI_E_DEVICE, "sweep launch (light group): %s", hipGetErrorString(e));
        }
        HIP_TRY(hipEventRecord(h->ev_join, h->stream2));
        HIP_TRY(hipStreamWaitEvent(st, h->ev_join, 0));
        // re-arm the start gate only here: `st` has now joined BOTH gated consumers (its own wait and stream2's), so neither can
        // still be waiting for the value that is being reset
        if (vh > 0 && h->start_sig && !pl.ksplit) HIP_TRY(hipStreamWriteValue32(st, h->start_sig, 0, 0));
    }
    if (C > 1 || pl.split) {
        const long long steps = (a.n - a.n1 + 1) * (long long)a.K;
        if (pl.s2_ok) HIP_TRY(hipMemsetAsync(h->d_heavy_left.p, 0, 4, st));
        e = pmdi_launch_chain_order((const long long *)h->d_cost.p, (int *)h->d_lorder.p, a.stats,
                                    pl.split ? (unsigned char *)h->d_group.p : nullptr, pl.light_ids * steps, C, st,
                                    pl.s2_ok ? (const int *)h->d_handed.p : nullptr, h->sweep_no + 3 - pl.sticky,
                                    pl.s2_ok ? (int *)h->d_heavy_left.p : nullptr);
        if (e != hipSuccess) return fail(PMDI_E_DEVICE, "chain-order launch: %s", hipGetErrorString(e));
        h->have_order = true;
    }
    return PMDI_OK;
}

// ---- pmdi_create, in the order of its parts ----------------------------------------------------------------------------------

// dataset k on the device: the data row-major, the host-built tables of its cluster type, the chains' arenas
int upload_dataset(pmdi_handle *h, int k, const pmdi_dataset &src)
{
    const int N = h->cfg.N, P = h->cfg.P;
    const long long n = h->cfg.n, cap = h->cap;
    DsetDev &d = h->ds[k];
    int rc = 0;
    if (src.D < 1) return fail(PMDI_E_ARG, "dataset %d: D=%d", k, src.D);
    if (src.ld < n) return fail(PMDI_E_ARG, "dataset %d: ld=%lld < n. Datasets don't have same number of observations.", k, (long long)src.ld);
    d.kind = src.kind; d.D = src.D; d.L = 0; d.flag_off = h->sumD;
    h->sumD += src.D;
    if (src.D > h->Dmax) h->Dmax = src.D;
    const int D = src.D;
    if (src.kind == PMDI_GAUSSIAN) {
        if (!src.xf) return fail(PMDI_E_ARG, "dataset %d: xf is null", k);
        std::vector<double> x((size_t)n * D);
        for (long long i = 0; i < n; ++i)
            for (int q = 0; q < D; ++q) x[(size_t)i * D + q] = src.xf[(size_t)q * src.ld + i];
        if ((rc = upload(h, x, &d.xf))) return rc;
        // gaussian_cluster.jl:38-40 prefix and :76-79 constant, per cluster size
        std::vector<double> g((size_t)n + 1), lm((size_t)n + 1);
        for (long long m = 0; m <= n; ++m) {
            const double nn = (double)m;
            g[m] = (log(1.0 / sqrt(M_PI)) + lgamma(0.5 * nn + 1.0)) - lgamma(0.5 * nn + 0.5);
            const double a_n = (nn / 2.0 + 0.5), a_0 = 0.5, b_0 = 0.5, k_0 = 0.001, k_n = nn + k_0;
            lm[m] = (a_0 * log(b_0)) + lgamma(a_n) - lgamma(a_0) + 0.5 * (log(k_0) - log(k_n)) -
                    (nn * 0.5) * log(2.0 * M_PI);
        }
        if ((rc = upload(h, g, &d.gtab))) return rc;
        if ((rc = upload(h, lm, &d.lmtab))) return rc;
    } else if (src.kind == PMDI_CATEGORICAL || src.kind == PMDI_NEGBINOM) {
        if (!src.xi) return fail(PMDI_E_ARG, "dataset %d: xi is null", k);
        std::vector<int> x((size_t)n * D);
        std::vector<int> maxcol(D, 0);
        std::vector<long long> colsum(D, 0);
        long long gmax = 0;
        for (long long i = 0; i < n; ++i)
            for (int q = 0; q < D; ++q) {
                const long long v = src.xi[(size_t)q * src.ld + i];
                if (src.kind == PMDI_CATEGORICAL && v < 1) return fail(PMDI_E_DATA, "dataset %d: categorical level %lld < 1", k, v);
                if (src.kind == PMDI_NEGBINOM && v < 0) return fail(PMDI_E_DATA, "dataset %d: negative count %lld", k, v);
                if (v > 0x3fffffff) return fail(PMDI_E_DATA, "dataset %d: value %lld too large", k, v);
                x[(size_t)i * D + q] = (int)v;
                if (v > maxcol[q]) maxcol[q] = (int)v;
                if (v > gmax) gmax = v;
                colsum[q] += v;
            }
        if ((rc = upload(h, x, &d.xi))) return rc;
        if (src.kind == PMDI_CATEGORICAL) {
            if (gmax > 4096) return fail(PMDI_E_DATA, "dataset %d: %lld categorical levels (max 4096)", k, gmax);
            d.L = (int)gmax;                                  // categorical_cluster.jl:8
            if ((rc = upload(h, maxcol, &d.maxcol))) return rc;
            std::vector<double> lh((size_t)(2 * n + gmax + 3)), lgh((size_t)(2 * (n + gmax) + 3));
            for (size_t j = 0; j < lh.size(); ++j) lh[j] = log(0.5 * (double)j);
            for (size_t j = 0; j < lgh.size(); ++j) lgh[j] = lgamma(0.5 * (double)j);
            if ((rc = upload(h, lh, &d.lhtab))) return rc;
            if ((rc = upload(h, lgh, &d.lghtab))) return rc;
        } else {
            long long smax = 0;
            for (int q = 0; q < D; ++q) if (colsum[q] > smax) smax = colsum[q];
            const long long len = n + gmax + smax + 8;
            if (len > (1LL << 27)) return fail(PMDI_E_DATA, "dataset %d: NegBinom lgamma table of %lld entries is too large", k, len);
            std::vector<double> lg((size_t)len);
            for (long long m = 0; m < len; ++m) lg[m] = lgamma((double)m);
            if ((rc = upload(h, lg, &d.lgtab))) return rc;
            d.lgtab_len = len;
        }
    } else {
        return fail(PMDI_E_ARG, "dataset %d: unknown kind %d", k, src.kind);
    }
    d.stride = layout_arena(d, N, P, cap, n, true);
    void *arena = nullptr;
    if ((rc = dev_alloc(h, &arena, d.stride * (size_t)h->cfg.n_chains))) return rc;
    d.arena = (char *)arena;
    if (hipMemset(arena, 0, d.stride * (size_t)h->cfg.n_chains) != hipSuccess) return fail(PMDI_E_DEVICE, "hipMemset failed");
    return PMDI_OK;
}

// the streams and events of the heavy / light split, and the start gate's signal memory, as the plan asks
int create_launch_objects(pmdi_handle *h)
{
    if (!h->plan.split) return PMDI_OK;
    // the slow chains bound the launch, so their workgroups must not queue behind the many
    // light ones: light launch on a low-priority stream, heaviest chains on a high-priority one
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);      // (least, greatest); greatest is the smaller number
    if (hipStreamCreateWithPriority(&h->stream2, hipStreamNonBlocking, prio_lo) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) != hipSuccess ||
        hipStreamCreateWithPriority(&h->stream3, hipStreamNonBlocking, prio_hi) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_join3, hipEventDisableTiming) != hipSuccess)
        return fail(PMDI_E_DEVICE, "stream/event creation failed");
    void *sig = nullptr;
    if (h->plan.want_gate && hipExtMallocWithFlags(&sig, 8, hipMallocSignalMemory) == hipSuccess) {
        h->start_sig = (unsigned *)sig; h->owned.push_back(sig);
        (void)hipMemset(sig, 0, 8);
    }
    return PMDI_OK;
}

// per-chain state and scratch of the sweep launches
int alloc_sweep_state(pmdi_handle *h)
{
    const int K = h->cfg.K, P = h->cfg.P;
    const long long n = h->cfg.n;
    int rc = 0;
    const int C = h->cfg.n_chains;
    for (DevBuf &b : h->d_args) if ((rc = b.ensure(sizeof(SweepArgs)))) return rc;
    if ((rc = h->d_usc.ensure((size_t)C * K * P * 8)) || (rc = h->d_partstar.ensure((size_t)C * K * P * 4)) ||
        (rc = h->d_kstate.ensure((size_t)C * PMDI_KMAX_I * 2 * 4)) || (rc = h->d_err.ensure((size_t)C * 4)) ||
        (rc = h->d_stats.ensure((size_t)C * 8 * 8)) || (rc = h->d_pstar.ensure((size_t)C * 4)) ||
        (rc = h->d_phase.ensure((size_t)C * 16 * 8)) ||
        (rc = h->d_cost.ensure((size_t)C * 8)) || (rc = h->d_work.ensure((size_t)C * PMDI_KMAX_I * 8 * 8)) || (rc = h->d_lorder.ensure((size_t)C * 4)) || (rc = h->d_ticket.ensure(((size_t)C + 1) * 4)) ||
        (rc = h->d_group.ensure((size_t)C)) || (rc = h->d_requeue.ensure((size_t)C * 4)) ||
        (rc = h->d_requeue_total.ensure(4 * 8)) || (rc = h->d_handed.ensure((size_t)C * 4)) || (rc = h->d_swept_by.ensure((size_t)C * 4)) ||
        (rc = h->d_resume.ensure((size_t)C * 16 * 4)))
        return rc;
    if (hipMemset(h->d_swept_by.p, 0, (size_t)C * 4) != hipSuccess) return fail(PMDI_E_DEVICE, "hipMemset failed");
    {
        std::vector<int> never((size_t)C, -1000);
        if (hipMemcpy(h->d_handed.p, never.data(), (size_t)C * 4, hipMemcpyHostToDevice) != hipSuccess) return fail(PMDI_E_DEVICE, "memcpy failed");
    }
    if (hipMemset(h->d_requeue.p, 0, (size_t)C * 4) != hipSuccess || hipMemset(h->d_requeue_total.p, 0, 32) != hipSuccess)
        return fail(PMDI_E_DEVICE, "hipMemset failed");
    if (h->plan.want_xchg && ((rc = h->d_xcnt.ensure((size_t)C * 32 * 4)) || (rc = h->d_xinc.ensure((size_t)C * 2 * K * P * 8)) ||
                      (rc = h->d_xlab.ensure((size_t)C * 2 * K * P * 4)) || (rc = h->d_xhdr.ensure((size_t)C * 2 * K * 16))))
        return rc;
    if (h->cfg.q2_mode == 1 &&       // ancestor log of the resampling events: up to one per swept observation
        ((rc = h->d_anclog.ensure((size_t)C * (size_t)n * P * 4)) || (rc = h->d_evpos.ensure((size_t)C * 2 * (size_t)n * 4))))
        return rc;
    // first sweep: every chain is heavy (PMDI_SETTLED=2: every chain starts on the settled-chain kernel -- tests of its hand-back path)
    const bool all_heavy = !(h->plan.s2_ok && h->tun.settled == 2);
    if (hipMemset(h->d_group.p, all_heavy ? 1 : 0, (size_t)C) != hipSuccess)
        return fail(PMDI_E_DEVICE, "hipMemset failed");
    // ... and that many heavy workgroups the first sweep waits for before a settled-chain workgroup keeps its slot
    const int heavy_first = all_heavy ? C : 0;
    if ((rc = h->d_heavy_left.ensure(4))) return rc;
    if (hipMemcpy(h->d_heavy_left.p, &heavy_first, 4, hipMemcpyHostToDevice) != hipSuccess) return fail(PMDI_E_DEVICE, "memcpy failed");
    if (h->plan.phase_on) {
        if ((rc = h->d_stamp.ensure((size_t)C * 2 * 8))) return rc;
        if (hipMemset(h->d_stamp.p, 0, (size_t)C * 2 * 8) != hipSuccess) return fail(PMDI_E_DEVICE, "hipMemset failed");
    }
    return PMDI_OK;
}

// pinned staging ring of the argument blocks (asynchronous launches); without it the copies fall back to pageable memory
void alloc_staging_ring(pmdi_handle *h)
{
    void *ring = nullptr;
    if (hipHostMalloc(&ring, sizeof(SweepArgs) * pmdi_handle::RING, hipHostMallocDefault) == hipSuccess) {
        h->ring = (SweepArgs *)ring;
        for (int i = 0; i < pmdi_handle::RING; ++i)
            if (hipEventCreateWithFlags(&h->ring_ev[i], hipEventDisableTiming) != hipSuccess) {
                for (int j = 0; j < i; ++j) { (void)hipEventDestroy(h->ring_ev[j]); h->ring_ev[j] = nullptr; }
                (void)hipHostFree(ring); h->ring = nullptr;
                break;
            }
    }
}

// null-cluster marginal (src/pmdi.jl:120-128): all rows in one cluster, all features on
int null_marginal(pmdi_handle *h)
{
    const int K = h->cfg.K, N = h->cfg.N, C = h->cfg.n_chains;
    const long long n = h->cfg.n;
    int rc = 0;
    std::vector<int> traj((size_t)K * n, 0);
    if ((rc = h->d_traj.ensure((size_t)C * K * n * 4)) || (rc = h->d_lm.ensure((size_t)C * h->sumD * N * 8)) ||
        (rc = h->d_firstpos.ensure((size_t)C * K * N * 4)) || (rc = h->d_fnull.ensure((size_t)h->sumD * 8)) ||
        (rc = h->d_fflags.ensure((size_t)C * h->sumD)) || (rc = h->d_fprob.ensure((size_t)C * h->sumD * 8)))
        return rc;
    if (hipMemcpy(h->d_traj.p, traj.data(), traj.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return fail(PMDI_E_DEVICE, "memcpy failed");
    std::vector<double> zero((size_t)h->sumD, 0.0);
    if (hipMemcpy(h->d_fnull.p, zero.data(), zero.size() * 8, hipMemcpyHostToDevice) != hipSuccess) return fail(PMDI_E_DEVICE, "memcpy failed");
    FeatSelArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.K = K; fa.N = 1; fa.sumD = h->sumD; fa.n = n; fa.iter = 0; fa.seed = h->cfg.seed;
    for (int k = 0; k < K; ++k) fa.ds[k] = h->ds[k];
    fa.traj = (const int *)h->d_traj.p; fa.lm = (double *)h->d_lm.p; fa.firstpos = (int *)h->d_firstpos.p;
    fa.fnull = (const double *)h->d_fnull.p; fa.flags_out = (unsigned char *)h->d_fflags.p; fa.prob_out = (double *)h->d_fprob.p;
    hipError_t e = pmdi_launch_featsel(fa, 1, h->stream);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "null-marginal launch: %s", hipGetErrorString(e));
    if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(PMDI_E_DEVICE, "null-marginal kernel failed");
    std::vector<double> lm((size_t)h->sumD);
    if (hipMemcpy(lm.data(), h->d_lm.p, lm.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return fail(PMDI_E_DEVICE, "memcpy failed");
    for (double &v : lm) v = -v;                               // featureNull = -calc_logmarginal (:127)
    if (hipMemcpy(h->d_fnull.p, lm.data(), lm.size() * 8, hipMemcpyHostToDevice) != hipSuccess) return fail(PMDI_E_DEVICE, "memcpy failed");
    return PMDI_OK;
}

}  // namespace

extern "C" {

const char *pmdi_last_error(void) { return g_err; }

void pmdi_tuning_default(pmdi_tuning *t)
{
    if (!t) return;
    int32_t *f = (int32_t *)t;
    for (size_t i = 0; i < sizeof(pmdi_tuning) / sizeof(int32_t); ++i) f[i] = -1;
}

// The one place of the library that reads the environment -- and only when a caller asks for it.
void pmdi_tuning_from_env(pmdi_tuning *t)
{
    if (!t) return;
    pmdi_tuning_default(t);
    auto env = [](const char *name, int32_t &field) { const char *v = getenv(name); if (v && *v) field = (int32_t)atoi(v); };
    env("PMDI_SETTLED", t->settled); env("PMDI_CONTINUE", t->continue_inplace); env("PMDI_STICKY", t->sticky);
    env("PMDI_LIGHT_IDS", t->light_ids); env("PMDI_S2_COLS", t->s2_cols); env("PMDI_S2_IDCAP", t->s2_idcap); env("PMDI_S2_CLS", t->s2_cls);
    env("PMDI_KSPLIT", t->ksplit); env("PMDI_REQUEUE_KSPLIT", t->requeue_ksplit); env("PMDI_SPLIT", t->split);
    env("PMDI_HEAVY_T", t->heavy_threads); env("PMDI_TWO_PER_CU", t->two_per_cu); env("PMDI_VERY_HEAVY", t->very_heavy);
    env("PMDI_START_GATE", t->start_gate); env("PMDI_TICKET", t->ticket); env("PMDI_TERMS_CAP", t->terms_cap); env("PMDI_LDS_TARGET", t->lds_target);
    env("PMDI_HOLD", t->hold); env("PMDI_SWEEP_GRID", t->sweep_grid);
    if (getenv("PMDI_PHASE_TIMERS")) t->phase_timers = 1;
    auto has = [](const char *name, const char *what) { const char *v = getenv(name); return v && strstr(v, what) != nullptr; };
    t->profiled = (has("LD_PRELOAD", "rocprof") || has("ROCP_TOOL_LIBRARIES", "rocprof") || has("HSA_TOOLS_LIB", "rocprof")) ? 1 : 0;
}
int pmdi_abi_version(void) { return PMDI_ABI_VERSION; }

int pmdi_destroy(pmdi_handle *h)
{
    if (!h) return PMDI_OK;
    if (h->children > 0)
        return fail(PMDI_E_STATE, "pmdi_destroy: %d object(s) created from this handle (pmdi_gibbs_create / pmdi_clusters_new) are still alive", h->children);
    (void)hipSetDevice(h->cfg.device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    (void)hipDeviceSynchronize();
    for (int i = 0; i < pmdi_handle::RING; ++i) if (h->ring_ev[i]) (void)hipEventDestroy(h->ring_ev[i]);
    if (h->ring) (void)hipHostFree(h->ring);
    for (void *p : h->owned) (void)hipFree(p);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    if (h->stream2) { (void)hipStreamSynchronize(h->stream2); (void)hipStreamDestroy(h->stream2); }
    if (h->stream3) { (void)hipStreamSynchronize(h->stream3); (void)hipStreamDestroy(h->stream3); }
    if (h->ev_join3) (void)hipEventDestroy(h->ev_join3);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->ev_join) (void)hipEventDestroy(h->ev_join);
    delete h;                   // (frees every DevBuf of the handle: its device is current)
    return PMDI_OK;
}

int pmdi_create(const pmdi_config *cfg, const pmdi_dataset *datasets, pmdi_handle **out)
{
    if (!cfg || !datasets || !out) return fail(PMDI_E_ARG, "null argument");
    *out = nullptr;
    if (cfg->abi_version != PMDI_ABI_VERSION) return fail(PMDI_E_ARG, "abi_version %d != %d", cfg->abi_version, PMDI_ABI_VERSION);
    const int K = cfg->K, N = cfg->N, P = cfg->P;
    const long long n = cfg->n;
    // the @asserts of src/pmdi.jl:50-55 that concern this path
    if (K < 1 || K > PMDI_KMAX_I) return fail(PMDI_E_ARG, "K=%d outside 1..%d", K, PMDI_KMAX_I);
    if (n < 2 || n > 0x7fffffffLL / 4) return fail(PMDI_E_ARG, "n=%lld out of range", n);
    if (!(N <= n && N > 1)) return fail(PMDI_E_ARG, "Number of clusters must be greater than 1 and not greater than the number of observations");
    if (N > 255) return fail(PMDI_E_ARG, "N=%d: this build supports N <= 255 (labels travel as bytes; the mutation CDF of a particle class is formed by one wave, up to four labels per lane, pairwise beyond 128 like Base.cumsum)", N);
    if (P < 2) return fail(PMDI_E_ARG, "Conditional particle filter requires 2 or more particles");
    if (P > 1048575) return fail(PMDI_E_ARG, "P=%d too large", P);
    if (cfg->n_chains < 1) return fail(PMDI_E_ARG, "n_chains must be >= 1");
    if (cfg->q1_mode < 0 || cfg->q1_mode > 1) return fail(PMDI_E_ARG, "q1_mode must be 0 or 1");
    if (cfg->q2_mode < 0 || cfg->q2_mode > 1) return fail(PMDI_E_ARG, "q2_mode must be 0 or 1");
    long long cap = cfg->pool_cap > 0 ? cfg->pool_cap : (long long)N * P + 1;
    if (cap > (long long)N * P + 1) cap = (long long)N * P + 1;
    if (cap < N + 2) return fail(PMDI_E_ARG, "pool_cap too small");

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(PMDI_E_DEVICE, "no HIP device visible (this library has no CPU path)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(PMDI_E_DEVICE, "device %d not in 0..%d", cfg->device, ndev - 1);
    HIP_TRY(hipSetDevice(cfg->device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, cfg->device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(PMDI_E_DEVICE, "device %d is %s; the kernels are built for gfx950 only", cfg->device, prop.gcnArchName);

    pmdi_handle *h = new (std::nothrow) pmdi_handle();
    if (!h) return fail(PMDI_E_MEMORY, "out of host memory");
    h->cfg = *cfg;
    if (cfg->tuning) h->tun = *cfg->tuning; else pmdi_tuning_default(&h->tun);
    h->cfg.tuning = nullptr;
    h->cap = cap;
    h->npairs = K > 1 ? K * (K - 1) / 2 : 1;
    int rc = 0;
    auto bail = [&](int code) { pmdi_destroy(h); return code; };
    {   // the settled-chain launch: do its workgroups keep their slots, and how many are there (pmdi_tuning::hold, sweep_grid)
        const int hold = h->tun.hold < 0 ? 1 : h->tun.hold, grid = h->tun.sweep_grid;
        if (hold > 2) return bail(fail(PMDI_E_ARG, "tuning.hold=%d outside 0..2", hold));
        if (grid == 0 || grid < -1) return bail(fail(PMDI_E_ARG, "tuning.sweep_grid=%d: at least one workgroup", grid));
        h->hold = h->tun.ticket != 0 ? hold : 0;        // (slots are kept by drawing again: no ticket, no draw)
        if (h->hold == 0 && grid > 0 && grid < cfg->n_chains)
            return bail(fail(PMDI_E_ARG, "tuning.sweep_grid=%d < n_chains=%d with one-shot workgroups (hold = 0, or no ticket): chains would stay unswept", grid, cfg->n_chains));
        h->sweep_grid = (h->hold == 2 && grid > 0 && grid < cfg->n_chains) ? grid : cfg->n_chains;
    }
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) return bail(fail(PMDI_E_DEVICE, "hipStreamCreate failed"));

    for (int k = 0; k < K; ++k)
        if ((rc = upload_dataset(h, k, datasets[k]))) return bail(rc);
    PlanDevice dev;              // what the plan needs to know about the device
    dev.cus = prop.multiProcessorCount;
    int can_wait = 0;
    (void)hipDeviceGetAttribute(&can_wait, hipDeviceAttributeCanUseStreamWaitValue, cfg->device);
    dev.wait_value = can_wait != 0;
    dev.blocks_per_cu = [](const SweepArgs &a, int T) { int blocks = 0; return pmdi_sweep_blocks_per_cu(a, T, &blocks) == hipSuccess ? blocks : 0; };
    if ((rc = pmdi_plan_sweep(h->cfg, h->tun, h->Dmax, cap, dev, &h->plan)) ||
        (rc = create_launch_objects(h)) || (rc = alloc_sweep_state(h)))
        return bail(rc);
    alloc_staging_ring(h);
    if ((rc = null_marginal(h))) return bail(rc);
    *out = h;
    return PMDI_OK;
}

int pmdi_phase_timers(pmdi_handle *h, int32_t chain, int64_t *out16)
{
    if (!h || !out16 || chain < 0 || chain >= h->cfg.n_chains) return fail(PMDI_E_ARG, "bad argument");
    if (!h->plan.phase_on) return fail(PMDI_E_STATE, "set PMDI_PHASE_TIMERS=1 before pmdi_create");
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out16, (char *)h->d_phase.p + (size_t)chain * 16 * 8, 16 * 8, hipMemcpyDeviceToHost));
    return PMDI_OK;
}

int pmdi_chain_costs(pmdi_handle *h, int64_t *out)
{
    if (!h || !out) return fail(PMDI_E_ARG, "null argument");
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, h->d_cost.p, (size_t)h->cfg.n_chains * 8, hipMemcpyDeviceToHost));
    return PMDI_OK;
}
int pmdi_work_counters(pmdi_handle *h, int64_t *out)
{
    if (!h || !out) return fail(PMDI_E_ARG, "null argument");
    const int C = h->cfg.n_chains, K = h->cfg.K;
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(hipDeviceSynchronize());
    std::vector<long long> w((size_t)C * PMDI_KMAX_I * 8);
    HIP_TRY(hipMemcpy(w.data(), h->d_work.p, w.size() * 8, hipMemcpyDeviceToHost));
    for (int c = 0; c < C; ++c)
        for (int k = 0; k < K; ++k)
            for (int j = 0; j < 8; ++j) out[((size_t)c * K + k) * 8 + j] = w[((size_t)c * PMDI_KMAX_I + k) * 8 + j];
    return PMDI_OK;
}
int pmdi_block_threads(const pmdi_handle *h) { return h ? h->plan.T : 0; }
int pmdi_is_split(const pmdi_handle *h) { return h ? h->plan.ksplit : 0; }
int64_t pmdi_shader_clock_hz(const pmdi_handle *h)
{
    if (!h) return 0;
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeClockRate, h->cfg.device) != hipSuccess) return 0;
    return (int64_t)khz * 1000;
}
int64_t pmdi_lds_bytes(const pmdi_handle *h)
{
    if (!h) return 0;
    SweepArgs a;
    fill_sweep_common(h, a);
    return (int64_t)pmdi_sweep_lds_bytes(a, h->plan.T);
}
int pmdi_sweep_layout(const pmdi_handle *h, int32_t *out32)
{
    if (!h || !out32) return fail(PMDI_E_ARG, "null argument");
    pmdi_plan_layout32(h->plan, h->start_sig != nullptr, h->d_xcnt.p != nullptr, h->cfg.K, h->cfg.P, out32);
    return PMDI_OK;
}
int pmdi_settled_launch(pmdi_handle *h, int32_t *out4)
{
    if (!h || !out4) return fail(PMDI_E_ARG, "null argument");
    out4[0] = out4[1] = out4[2] = out4[3] = 0;
    if (!h->plan.s2_ok) return PMDI_OK;
    HIP_TRY(hipSetDevice(h->cfg.device));
    SweepArgs a;
    fill_sweep_common(h, a);
    pmdi_put_tables(h->plan.resume, a);         // (the launch asks for the larger of the two kernels' LDS layouts)
    int blocks = 0, cus = 0;
    HIP_TRY(pmdi_sweep2_blocks_per_cu(a, &blocks));
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->cfg.device));
    out4[0] = h->hold; out4[1] = h->sweep_grid; out4[2] = blocks * cus;
    if (h->tun.ticket != 0 && h->sweep_no > 0) {
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(&out4[3], h->d_ticket.p, 4, hipMemcpyDeviceToHost));
    }
    return PMDI_OK;
}
int pmdi_chain_stamps(pmdi_handle *h, int64_t *out)
{
    if (!h || !out) return fail(PMDI_E_ARG, "null argument");
    if (!h->plan.phase_on) return fail(PMDI_E_STATE, "set PMDI_PHASE_TIMERS=1 before pmdi_create");
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, h->d_stamp.p, (size_t)h->cfg.n_chains * 2 * 8, hipMemcpyDeviceToHost));
    return PMDI_OK;
}
int pmdi_sum_D(const pmdi_handle *h) { return h ? h->sumD : 0; }
int pmdi_settled_kernel(pmdi_handle *h, int64_t *given_back4)
{
    if (!h) return 0;
    if (given_back4) {
        given_back4[0] = given_back4[1] = given_back4[2] = given_back4[3] = 0;
        if (h->plan.s2_ok) {
            if (hipSetDevice(h->cfg.device) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
                hipMemcpy(given_back4, h->d_requeue_total.p, 32, hipMemcpyDeviceToHost) != hipSuccess)
                return fail(PMDI_E_DEVICE, "pmdi_settled_kernel: reading the counters failed");
        }
    }
    return h->plan.s2_ok ? 1 : 0;
}
int pmdi_chain_swept_by(pmdi_handle *h, int32_t *out)
{
    if (!h || !out) return fail(PMDI_E_ARG, "null argument");
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, h->d_swept_by.p, (size_t)h->cfg.n_chains * 4, hipMemcpyDeviceToHost));
    return PMDI_OK;
}
int64_t pmdi_pool_cap(const pmdi_handle *h) { return h ? h->cap : 0; }
int pmdi_categorical_L(const pmdi_handle *h, int32_t k) { return (h && k >= 0 && k < h->cfg.K) ? h->ds[k].L : 0; }

int pmdi_sweep_device(pmdi_handle *h, int64_t iter, const int32_t *s_in, const int32_t *order_obs, int64_t n1,
                      const double *Pi, const double *log1p_phi, const uint8_t *feature_flag, double lw_init,
                      int32_t *s_out, double *logweight, int32_t *p_star, int64_t *stats, int32_t *err, void *stream)
{
    if (!h || !s_in || !order_obs || !Pi || !log1p_phi || !s_out) return fail(PMDI_E_ARG, "null argument");
    if (n1 < 1 || n1 > h->cfg.n) return fail(PMDI_E_ARG, "n1=%lld outside 1..n (rho*n < 1 is undefined in the reference)", (long long)n1);
    HIP_TRY(hipSetDevice(h->cfg.device));
    SweepArgs a;
    fill_sweep_call(h, a, iter, n1, lw_init, s_in, order_obs, Pi, log1p_phi, feature_flag, s_out, logweight, p_star, (long long *)stats, err, nullptr);
    hipStream_t st = (hipStream_t)stream;   // used verbatim: NULL is the device's default (null) stream
    const int lrc = launch_sweep_groups(h, a, st);
    if (lrc) return lrc;
    h->swept = true; h->last_n1 = n1;
    return PMDI_OK;
}

int pmdi_psm_counts_device(int32_t device, const uint8_t *samples, int64_t S, int32_t K, int64_t n,
                           int64_t row_lo, int64_t row_hi, int32_t n_labels, int32_t *counts, void *stream)
{
    if (!samples || !counts) return fail(PMDI_E_ARG, "null argument");
    if (S < 1 || K < 1 || n < 1 || row_lo < 0 || row_hi > n || row_lo > row_hi)
        return fail(PMDI_E_ARG, "S=%lld K=%d n=%lld rows [%lld, %lld): out of range", (long long)S, K, (long long)n,
                    (long long)row_lo, (long long)row_hi);
    if (S > 2147483647LL) return fail(PMDI_E_ARG, "S=%lld samples overflow the int32 counts", (long long)S);
    if ((n + 63) / 64 > 2147483647LL || (row_hi - row_lo + 63) / 64 > 65535 || K > 65535)
        return fail(PMDI_E_ARG, "grid too large: split the rows into blocks of at most 4194240");
    HIP_TRY(hipSetDevice(device));
    if (n_labels < 0 || n_labels > 256) return fail(PMDI_E_ARG, "n_labels=%d outside 0..256", n_labels);
    // labels known to be < 64: one-hot int8 GEMM on the matrix cores; otherwise byte compares on the vector ALUs
    const bool mfma = n_labels >= 1 && n_labels <= 64 && (row_hi - row_lo + 127) / 128 <= 65535;
    hipError_t e = mfma ? pmdi_launch_psm_counts_mfma(samples, S, K, n, row_lo, row_hi, n_labels, counts, (hipStream_t)stream)
                        : pmdi_launch_psm_counts(samples, S, K, n, row_lo, row_hi, counts, (hipStream_t)stream);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "psm-count launch: %s", hipGetErrorString(e));
    return PMDI_OK;
}

int pmdi_psm_score_device(int32_t device, const int32_t *counts, int64_t S, int32_t K, int64_t n, int32_t which,
                          const int32_t *cand, int64_t B, int64_t ld, int64_t *agree_out, int64_t *pairs_out, int64_t *total_out,
                          void *stream)
{
    if (!counts || !cand || !agree_out || !pairs_out || !total_out) return fail(PMDI_E_ARG, "pmdi_psm_score_device: null argument");
    const int rc = pmdi_psm_shared_args("pmdi_psm_score_device", S, K, n, which, true, B, ld);
    if (rc) return rc;
    const unsigned __int128 P = (unsigned __int128)(n * (n - 1) / 2);
    const unsigned __int128 D = psm_divisor(S, K, which);
    if (D * P >= ((unsigned __int128)1 << 62))       // D pairs + total and every other sum of the criteria stay inside int64
        return fail(PMDI_E_ARG, "pmdi_psm_score_device: S=%lld with n=%lld: D n (n - 1) / 2 >= 2^62", (long long)S, (long long)n);
    if (n == 1) {                                    // no pairs
        for (int64_t b = 0; b < B; ++b) agree_out[b] = pairs_out[b] = 0;
        *total_out = 0;
        return PMDI_OK;
    }
    HIP_TRY(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    Scratch out;
    const size_t bytes = ((size_t)2 * B + 1) * sizeof(unsigned long long);
    HIP_TRY(hipMalloc(&out.p, bytes));
    HIP_TRY(hipMemsetAsync(out.p, 0, bytes, st));
    const hipError_t e = pmdi_launch_psm_score(counts, K, n, which, D > ((unsigned __int128)1 << 22) ? 1 : 0, cand, B, ld,
                                               (unsigned long long *)out.p, st);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "psm-score launch: %s", hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(agree_out, out.p, (size_t)B * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(pairs_out, (const char *)out.p + (size_t)B * 8, (size_t)B * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(total_out, (const char *)out.p + (size_t)B * 16, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PMDI_OK;
}

int pmdi_psm_rowscore_device(int32_t device, const int32_t *counts, int64_t S, int32_t K, int64_t n, int32_t which,
                             const int32_t *cand, int64_t B, int64_t ld, int64_t *own_out, int32_t *size_out, int64_t *rowtotal_out,
                             void *stream)
{
    if (!counts || !cand || !own_out || !size_out || !rowtotal_out) return fail(PMDI_E_ARG, "pmdi_psm_rowscore_device: null argument");
    const int rc = pmdi_psm_shared_args("pmdi_psm_rowscore_device", S, K, n, which, true, B, ld);
    if (rc) return rc;
    const unsigned __int128 D = psm_divisor(S, K, which);
    if (D * (unsigned __int128)(n - 1) >= ((unsigned __int128)1 << 62))       // own and rowtotal stay inside int64
        return fail(PMDI_E_ARG, "pmdi_psm_rowscore_device: S=%lld with n=%lld: D (n - 1) >= 2^62", (long long)S, (long long)n);
    HIP_TRY(hipSetDevice(device));
    const hipError_t e = pmdi_launch_psm_rowscore(counts, K, n, which, D > ((unsigned __int128)1 << 22) ? 1 : 0, cand, B, ld,
                                                  (unsigned long long *)own_out, size_out, (unsigned long long *)rowtotal_out,
                                                  (hipStream_t)stream);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "psm-rowscore launch: %s", hipGetErrorString(e));
    return PMDI_OK;
}

static_assert(PMDI_REFINE_GMAX == PMDI_REFINE_GMAX_I, "the header's slot count is the kernels'");

int pmdi_psm_refine_device(int32_t device, const int32_t *counts, int64_t S, int32_t K, int64_t n, int32_t which,
                           const int32_t *start, int64_t B, int64_t ld, int32_t max_sweeps, int32_t *labels_out, int64_t *moves_out,
                           int32_t *sweeps_out, void *stream)
{
    if (!counts || !start || !labels_out || !moves_out || !sweeps_out) return fail(PMDI_E_ARG, "pmdi_psm_refine_device: null argument");
    const int rc = pmdi_psm_shared_args("pmdi_psm_refine_device", S, K, n, which, true, B, ld);
    if (rc) return rc;
    const unsigned __int128 D = psm_divisor(S, K, which);
    if (D > 2147483647u)                             // a w fits the uint32 work matrix and a gain fits int64 with room to spare
        return fail(PMDI_E_ARG, "pmdi_psm_refine_device: S=%lld: D > 2^31 - 1", (long long)S);
    if (max_sweeps < 1) return fail(PMDI_E_ARG, "pmdi_psm_refine_device: max_sweeps=%d < 1", max_sweeps);
    HIP_TRY(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    Scratch work, out;
    const size_t out_bytes = (size_t)B * 12 + 8;     // B moves, B sweeps, the flag
    HIP_TRY(hipMalloc(&work.p, (size_t)n * (size_t)n * 4));
    HIP_TRY(hipMalloc(&out.p, out_bytes));
    HIP_TRY(hipMemsetAsync(out.p, 0, out_bytes, st));
    long long *d_moves = (long long *)out.p;
    int *d_sweeps = (int *)((char *)out.p + (size_t)B * 8), *d_flag = d_sweeps + B;
    const hipError_t e = pmdi_launch_psm_refine(counts, K, n, which, (long long)D, D * (unsigned __int128)n >= ((unsigned __int128)1 << 32) ? 1 : 0,
                                                (unsigned *)work.p, start, B, ld, max_sweeps, labels_out, d_moves, d_sweeps, d_flag, st);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "psm-refine launch: %s", hipGetErrorString(e));
    int bad = 0;
    HIP_TRY(hipMemcpyAsync(moves_out, d_moves, (size_t)B * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(sweeps_out, d_sweeps, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&bad, d_flag, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));               // the work matrix is freed on return
    if (bad) return fail(PMDI_E_DATA, "pmdi_psm_refine_device: a start label outside 0..%d", PMDI_REFINE_GMAX - 1);
    return PMDI_OK;
}

int pmdi_vi_log2_table(int32_t *out)
{
    if (!out) return fail(PMDI_E_ARG, "pmdi_vi_log2_table: null argument");
    pmdi_vi_log2_table_host(out);
    return PMDI_OK;
}

int pmdi_psm_refine_vi_device(int32_t device, const int32_t *counts, int64_t S, int32_t K, int64_t n, int32_t which,
                              const int32_t *start, int64_t B, int64_t ld, int32_t max_sweeps, int32_t *labels_out, int64_t *moves_out,
                              int32_t *sweeps_out, int64_t *objective_out, void *stream)
{
    if (!counts || !start || !labels_out || !moves_out || !sweeps_out || !objective_out)
        return fail(PMDI_E_ARG, "pmdi_psm_refine_vi_device: null argument");
    const int rc = pmdi_psm_shared_args("pmdi_psm_refine_vi_device", S, K, n, which, true, B, ld);
    if (rc) return rc;
    const unsigned __int128 D = psm_divisor(S, K, which);
    if (D > 2147483647u)                             // a w fits the uint32 work matrix; own + D < 2^47 and every gain stays below 2^55
        return fail(PMDI_E_ARG, "pmdi_psm_refine_vi_device: S=%lld: D > 2^31 - 1", (long long)S);
    if (max_sweeps < 1) return fail(PMDI_E_ARG, "pmdi_psm_refine_vi_device: max_sweeps=%d < 1", max_sweeps);
    HIP_TRY(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    Scratch work, own, out;
    const size_t out_bytes = (size_t)B * 20 + 8;     // B moves, B objectives, B sweeps, the flag
    HIP_TRY(hipMalloc(&work.p, (size_t)n * (size_t)n * 4));
    HIP_TRY(hipMalloc(&own.p, (size_t)B * (size_t)n * 8));
    HIP_TRY(hipMalloc(&out.p, out_bytes));
    HIP_TRY(hipMemsetAsync(out.p, 0, out_bytes, st));
    long long *d_moves = (long long *)out.p, *d_obj = d_moves + B;
    int *d_sweeps = (int *)(d_obj + B), *d_flag = d_sweeps + B;
    const hipError_t e = pmdi_launch_psm_refine_vi(counts, K, n, which, (long long)D, (unsigned *)work.p, (long long *)own.p, start, B, ld,
                                                   max_sweeps, labels_out, d_moves, d_sweeps, d_obj, d_flag, st);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "psm-refine-vi launch: %s", hipGetErrorString(e));
    int bad = 0;
    HIP_TRY(hipMemcpyAsync(moves_out, d_moves, (size_t)B * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(objective_out, d_obj, (size_t)B * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(sweeps_out, d_sweeps, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&bad, d_flag, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));               // the work spaces are freed on return
    if (bad) return fail(PMDI_E_DATA, "pmdi_psm_refine_vi_device: a start label outside 0..%d", PMDI_REFINE_GMAX - 1);
    return PMDI_OK;
}

int pmdi_partition_rows_device(int32_t device, const void *labels, int32_t is_bytes, int64_t R, int64_t n, int64_t ld, int32_t G,
                               uint8_t *bytes_out, int64_t *pairs_out, int64_t *hl_out, int32_t *nclust_out, void *stream)
{
    if (!labels || !bytes_out || !pairs_out || !hl_out || !nclust_out) return fail(PMDI_E_ARG, "pmdi_partition_rows_device: null argument");
    if (R < 1 || R > 2147483647LL || n < 1 || n > 65535 || ld < n || G < 1 || G > PMDI_PARTDIST_GMAX)
        return fail(PMDI_E_ARG, "pmdi_partition_rows_device: R=%lld n=%lld ld=%lld G=%d out of range (R <= 2^31 - 1, 1 <= n <= 65535, ld >= n, 1 <= G <= %d)",
                    (long long)R, (long long)n, (long long)ld, G, PMDI_PARTDIST_GMAX);
    HIP_TRY(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    Scratch out;
    const size_t bytes = (size_t)R * 20 + 8;         // R pairs, R hl, R nclust, the flag
    HIP_TRY(hipMalloc(&out.p, bytes));
    HIP_TRY(hipMemsetAsync(out.p, 0, bytes, st));
    long long *d_pairs = (long long *)out.p, *d_hl = d_pairs + R;
    int *d_nclust = (int *)(d_hl + R), *d_flag = d_nclust + R;
    const hipError_t e = pmdi_launch_partition_rows(labels, is_bytes ? 1 : 0, R, n, ld, G, bytes_out, d_pairs, d_hl, d_nclust, d_flag, st);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "partition-rows launch: %s", hipGetErrorString(e));
    int bad = 0;
    HIP_TRY(hipMemcpyAsync(pairs_out, d_pairs, (size_t)R * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(hl_out, d_hl, (size_t)R * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(nclust_out, d_nclust, (size_t)R * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&bad, d_flag, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (bad) return fail(PMDI_E_ARG, "pmdi_partition_rows_device: a label outside 0..%d", G - 1);
    return PMDI_OK;
}

int pmdi_partition_distance_device(int32_t device, const uint8_t *cand_bytes, int64_t B, int32_t Gc, const uint8_t *draw_bytes, int64_t R,
                                   int32_t Gd, int64_t n, int64_t *both_out, int64_t *jl_out, void *stream)
{
    if (!cand_bytes || !draw_bytes || !both_out || !jl_out) return fail(PMDI_E_ARG, "pmdi_partition_distance_device: null argument");
    if (B < 1 || R < 1 || R > 2147483647LL || n < 1 || n > 65535 || Gc < 1 || Gc > PMDI_PARTDIST_GMAX || Gd < 1 || Gd > PMDI_PARTDIST_GMAX)
        return fail(PMDI_E_ARG, "pmdi_partition_distance_device: B=%lld R=%lld n=%lld Gc=%d Gd=%d out of range (R <= 2^31 - 1, 1 <= n <= 65535, 1 <= G <= %d)",
                    (long long)B, (long long)R, (long long)n, Gc, Gd, PMDI_PARTDIST_GMAX);
    if ((unsigned __int128)B * (unsigned __int128)R >= ((unsigned __int128)1 << 59))      // 8 B R bytes of each output
        return fail(PMDI_E_ARG, "pmdi_partition_distance_device: B=%lld R=%lld: B R >= 2^59", (long long)B, (long long)R);
    HIP_TRY(hipSetDevice(device));
    const hipError_t e = pmdi_launch_partition_distance(cand_bytes, B, Gc, draw_bytes, R, Gd, n, (long long *)both_out, (long long *)jl_out,
                                                        (hipStream_t)stream);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "partition-distance launch: %s", hipGetErrorString(e));
    return PMDI_OK;
}

int pmdi_partition_refine_device(int32_t device, const uint8_t *draw_bytes, int64_t R, int32_t Gd, int64_t n, const int32_t *start, int64_t B,
                                 int64_t ld, int32_t gcap, int32_t loss, int32_t max_sweeps, int32_t *labels_out, int64_t *moves_out,
                                 int32_t *sweeps_out, int32_t *converged_out, int64_t *marginal_out, int64_t *joint_out, void *stream)
{
    if (!draw_bytes || !start || !labels_out || !moves_out || !sweeps_out || !converged_out || !marginal_out || !joint_out)
        return fail(PMDI_E_ARG, "pmdi_partition_refine_device: null argument");
    if (B < 1 || R < 1 || R > (1LL << 24) || n < 1 || n > 65535 || R * n >= (1LL << 28) || ld < n || Gd < 1 || Gd > PMDI_PARTDIST_GMAX ||
        gcap < 1 || gcap > PMDI_PARTDIST_GMAX)
        return fail(PMDI_E_ARG, "pmdi_partition_refine_device: B=%lld R=%lld n=%lld ld=%lld Gd=%d gcap=%d out of range (R <= 2^24, 1 <= n <= 65535, R n < 2^28, ld >= n, 1 <= Gd, gcap <= %d)",
                    (long long)B, (long long)R, (long long)n, (long long)ld, Gd, gcap, PMDI_PARTDIST_GMAX);
    if (loss != 0 && loss != 1) return fail(PMDI_E_ARG, "pmdi_partition_refine_device: loss=%d is not 0 (binder) or 1 (vi)", loss);
    if (max_sweeps < 1) return fail(PMDI_E_ARG, "pmdi_partition_refine_device: max_sweeps=%d < 1", max_sweeps);
    int lgp = 0;
    while ((1 << lgp) < gcap) ++lgp;                 // the slots of one (r, h), padded to a power of two
    const unsigned __int128 table_bytes = (unsigned __int128)B * (unsigned __int128)(((R * Gd) << lgp) * 2);
    if (table_bytes >= ((unsigned __int128)1 << 62))
        return fail(PMDI_E_MEMORY, "pmdi_partition_refine_device: B=%lld starts need tables of 2^62 bytes or more", (long long)B);
    HIP_TRY(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    Scratch transposed, tables, out;
    const size_t out_bytes = (size_t)B * 32 + 8;     // B moves, B marginals, B joints, B sweeps, B converged, the flag
    HIP_TRY(hipMalloc(&transposed.p, (size_t)n * (size_t)R));
    HIP_TRY(hipMalloc(&tables.p, (size_t)table_bytes));
    HIP_TRY(hipMalloc(&out.p, out_bytes));
    HIP_TRY(hipMemsetAsync(tables.p, 0, (size_t)table_bytes, st));
    HIP_TRY(hipMemsetAsync(out.p, 0, out_bytes, st));
    long long *d_moves = (long long *)out.p, *d_marginal = d_moves + B, *d_joint = d_marginal + B;
    int *d_sweeps = (int *)(d_joint + B), *d_converged = d_sweeps + B, *d_flag = d_converged + B;
    const hipError_t e = pmdi_launch_partition_refine(draw_bytes, R, Gd, n, (unsigned char *)transposed.p, (unsigned short *)tables.p, lgp, start,
                                                      B, ld, gcap, loss, max_sweeps, labels_out, d_moves, d_sweeps, d_converged, d_marginal,
                                                      d_joint, d_flag, st);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "partition-refine launch: %s", hipGetErrorString(e));
    int bad = 0;
    HIP_TRY(hipMemcpyAsync(moves_out, d_moves, (size_t)B * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(marginal_out, d_marginal, (size_t)B * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(joint_out, d_joint, (size_t)B * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(sweeps_out, d_sweeps, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(converged_out, d_converged, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&bad, d_flag, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));               // the work spaces are freed on return
    if (bad & 1) return fail(PMDI_E_DATA, "pmdi_partition_refine_device: a start label outside 0..%d", gcap - 1);
    if (bad & 2) return fail(PMDI_E_DATA, "pmdi_partition_refine_device: a draw label outside 0..%d", Gd - 1);
    return PMDI_OK;
}

static_assert(PMDI_BLOCKSUM_GMAX == PSM_BLOCKSUM_GMAX_I, "the header's group count is the kernel's");

int pmdi_psm_blocksum_device(int32_t device, const int32_t *counts, int64_t S, int32_t K, int64_t n, const int32_t *group, int32_t G,
                             int64_t *out, void *stream)
{
    if (!counts || !group || !out) return fail(PMDI_E_ARG, "pmdi_psm_blocksum_device: null argument");
    if (K < 1 || K > PMDI_KMAX || S < 1 || n < 1 || n > 65535 || G < 1 || G > PMDI_BLOCKSUM_GMAX)
        return fail(PMDI_E_ARG, "pmdi_psm_blocksum_device: S=%lld K=%d n=%lld G=%d out of range (K <= %d, n <= 65535, G <= %d)",
                    (long long)S, K, (long long)n, G, PMDI_KMAX, PMDI_BLOCKSUM_GMAX);
    if ((unsigned __int128)S * (unsigned)K * (unsigned __int128)(n * n) >= ((unsigned __int128)1 << 62))      // every sum stays inside int64
        return fail(PMDI_E_ARG, "pmdi_psm_blocksum_device: S=%lld with K=%d, n=%lld: S K n^2 >= 2^62", (long long)S, K, (long long)n);
    PsmBlocksumPlan plan;
    const long long bad = psm_blocksum_plan(group, n, G, plan);
    if (bad >= 0)
        return fail(PMDI_E_ARG, "pmdi_psm_blocksum_device: group[%lld]=%d outside 0..%d", bad, group[bad], G - 1);
    HIP_TRY(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    // one allocation: the labels (8-byte reads) first, then the int tables
    const int nchunks = plan.nchunks();
    const size_t o_perm = align_up(plan.g16.size() * 2, 16), o_at = o_perm + (size_t)n * 4, o_info = o_at + ((size_t)nchunks + 1) * 4,
                 o_size = o_info + (size_t)nchunks * 4, bytes = o_size + (size_t)G * 4;
    Scratch tab;
    HIP_TRY(hipMalloc(&tab.p, bytes));
    char *d = (char *)tab.p;
    HIP_TRY(hipMemcpyAsync(d, plan.g16.data(), plan.g16.size() * 2, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d + o_perm, plan.perm.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d + o_at, plan.chunk_at.data(), ((size_t)nchunks + 1) * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d + o_info, plan.chunk_info.data(), (size_t)nchunks * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d + o_size, plan.gsize.data(), (size_t)G * 4, hipMemcpyHostToDevice, st));
    const hipError_t e = pmdi_launch_psm_blocksum(counts, S, K, n, G, (const unsigned short *)d, plan.npad, (const int *)(d + o_perm),
                                                  (const int *)(d + o_at), (const int *)(d + o_info), nchunks, (const int *)(d + o_size),
                                                  (unsigned long long *)out, st);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "psm-blocksum launch: %s", hipGetErrorString(e));
    HIP_TRY(hipStreamSynchronize(st));               // the tables (and the plan they were copied from) are freed on return
    return PMDI_OK;
}

static_assert(PMDI_DATA_RAW == PMDI_DATA_RAW_I && PMDI_DATA_SQDEV == PMDI_DATA_SQDEV_I && PMDI_DATA_ZBIN == PMDI_DATA_ZBIN_I &&
                  PMDI_DATA_LEVELS == PMDI_DATA_LEVELS_I, "the header's modes are the kernels'");

int pmdi_data_groupsum_device(int32_t device, int32_t kind, const void *x, int64_t n, int32_t D, int64_t ld, const int32_t *group,
                              int32_t G, int32_t mode, const double *shift, const double *scale, int32_t L, void *out, void *stream)
{
    const char *who = "pmdi_data_groupsum_device";
    if (!x || !group || !out) return fail(PMDI_E_ARG, "%s: null argument", who);
    if (n < 1 || n > 65535 || D < 1 || D > 65535 || ld < D || G < 1 || G > PMDI_BLOCKSUM_GMAX)
        return fail(PMDI_E_ARG, "%s: n=%lld D=%d ld=%lld G=%d out of range (n, D <= 65535, ld >= D, G <= %d)", who, (long long)n, D,
                    (long long)ld, G, PMDI_BLOCKSUM_GMAX);
    if (kind != PMDI_GAUSSIAN && kind != PMDI_CATEGORICAL && kind != PMDI_NEGBINOM) return fail(PMDI_E_ARG, "%s: unknown kind %d", who, kind);
    if (mode != PMDI_DATA_RAW && mode != PMDI_DATA_SQDEV && mode != PMDI_DATA_ZBIN && mode != PMDI_DATA_LEVELS)
        return fail(PMDI_E_ARG, "%s: unknown mode %d", who, mode);
    const bool is_float = kind == PMDI_GAUSSIAN;
    if ((mode == PMDI_DATA_SQDEV || mode == PMDI_DATA_ZBIN) && !is_float)
        return fail(PMDI_E_ARG, "%s: mode %d needs Gaussian (Float64) data, not kind %d", who, mode, kind);
    if (mode == PMDI_DATA_LEVELS && kind != PMDI_CATEGORICAL) return fail(PMDI_E_ARG, "%s: PMDI_DATA_LEVELS needs Categorical data, not kind %d", who, kind);
    if (mode == PMDI_DATA_SQDEV && !shift) return fail(PMDI_E_ARG, "%s: PMDI_DATA_SQDEV without shift", who);
    if (mode == PMDI_DATA_ZBIN) {
        if (!shift || !scale) return fail(PMDI_E_ARG, "%s: PMDI_DATA_ZBIN without shift and scale", who);
        for (int d = 0; d < D; ++d)
            if (!std::isfinite(shift[d]) || !std::isfinite(scale[d]) || !(scale[d] > 0.0))
                return fail(PMDI_E_ARG, "%s: shift[%d]=%g, scale[%d]=%g: not finite, or scale <= 0", who, d, shift[d], d, scale[d]);
    }
    if (mode == PMDI_DATA_LEVELS && (L < 1 || L > 4096 || (long long)G * D * L > (1LL << 28)))
        return fail(PMDI_E_ARG, "%s: L=%d outside 1..4096, or G D L = %lld > 2^28", who, L, (long long)G * D * L);
    PsmBlocksumPlan plan;
    const long long bad = psm_blocksum_plan(group, n, G, plan);
    if (bad >= 0) return fail(PMDI_E_ARG, "%s: group[%lld]=%d outside 0..%d", who, bad, group[bad], G - 1);
    const int nchunks = plan.nchunks();
    const std::vector<int> chunks_at = data_groupsum_chunks_at(plan);      // the first chunk of every group
    HIP_TRY(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    const bool f_out = is_float && (mode == PMDI_DATA_RAW || mode == PMDI_DATA_SQDEV);
    const bool up_shift = mode == PMDI_DATA_SQDEV || mode == PMDI_DATA_ZBIN, up_scale = mode == PMDI_DATA_ZBIN;
    // one allocation: the doubles first, then the int tables (the plan's 16-bit label copies are not uploaded), then the flag
    const size_t o_scale = (size_t)D * 8, o_perm = 2 * (size_t)D * 8, o_at = o_perm + (size_t)n * 4, o_info = o_at + ((size_t)nchunks + 1) * 4,
                 o_gat = o_info + (size_t)nchunks * 4, o_flag = o_gat + ((size_t)G + 1) * 4, bytes = o_flag + 4;
    Scratch tab, part;
    HIP_TRY(hipMalloc(&tab.p, bytes));
    if (f_out) HIP_TRY(hipMalloc(&part.p, (size_t)nchunks * D * 8));
    char *d = (char *)tab.p;
    if (up_shift) HIP_TRY(hipMemcpyAsync(d, shift, (size_t)D * 8, hipMemcpyHostToDevice, st));
    if (up_scale) HIP_TRY(hipMemcpyAsync(d + o_scale, scale, (size_t)D * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d + o_perm, plan.perm.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d + o_at, plan.chunk_at.data(), ((size_t)nchunks + 1) * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d + o_info, plan.chunk_info.data(), (size_t)nchunks * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d + o_gat, chunks_at.data(), ((size_t)G + 1) * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d + o_flag, 0, 4, st));
    const hipError_t e = pmdi_launch_data_groupsum(is_float ? 1 : 0, x, D, ld, G, mode, (const int *)(d + o_perm), (const int *)(d + o_at),
                                                   (const int *)(d + o_info), nchunks, (const int *)(d + o_gat),
                                                   up_shift ? (const double *)d : nullptr, up_scale ? (const double *)(d + o_scale) : nullptr,
                                                   L, (double *)part.p, out, (int *)(d + o_flag), st);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "data-groupsum launch: %s", hipGetErrorString(e));
    int flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, d + o_flag, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));               // the tables and the partials are freed on return
    if (flag && mode == PMDI_DATA_ZBIN) return fail(PMDI_E_DATA, "%s: a non-finite element in PMDI_DATA_ZBIN", who);
    if (flag) return fail(PMDI_E_DATA, "%s: a level outside 1..%d in PMDI_DATA_LEVELS", who, L);
    return PMDI_OK;
}

int pmdi_label_counts_device(pmdi_handle *h, const int32_t *s, int32_t *counts, void *stream)
{
    if (!h || !s || !counts) return fail(PMDI_E_ARG, "null argument");
    HIP_TRY(hipSetDevice(h->cfg.device));
    hipError_t e = pmdi_launch_label_counts(s, counts, h->cfg.n_chains * h->cfg.K, h->cfg.n, h->cfg.N, (hipStream_t)stream);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "label-count launch: %s", hipGetErrorString(e));
    return PMDI_OK;
}

int pmdi_sweep(pmdi_handle *h, int64_t iter, const int64_t *s_in, const int64_t *order_obs, int64_t n1,
               const double *Pi, const double *Phi, const uint8_t *feature_flag, double lw_init, int64_t *s_out,
               double *logweight, int64_t *p_star, pmdi_sweep_stats *stats, double *trace)
{
    if (!h || !s_in || !order_obs || !Pi || !Phi) return fail(PMDI_E_ARG, "null argument");
    const int K = h->cfg.K, N = h->cfg.N, P = h->cfg.P, C = h->cfg.n_chains;
    const long long n = h->cfg.n;
    if (n1 < 1 || n1 > n) return fail(PMDI_E_ARG, "n1=%lld outside 1..n (rho*n < 1 is undefined in the reference)", (long long)n1);
    HIP_TRY(hipSetDevice(h->cfg.device));
    std::vector<int> s32((size_t)C * K * n), o32((size_t)C * n);
    for (size_t i = 0; i < s32.size(); ++i) {
        const long long v = s_in[i];
        if (v < 1 || v > N) return fail(PMDI_E_DATA, "s_in[%zu]=%lld outside 1..N", i, v);
        s32[i] = (int)(v - 1);
    }
    for (size_t i = 0; i < o32.size(); ++i) {
        const long long v = order_obs[i];
        if (v < 1 || v > n) return fail(PMDI_E_DATA, "order_obs[%zu]=%lld outside 1..n", i, v);
        o32[i] = (int)(v - 1);
    }
    std::vector<double> lphi((size_t)C * h->npairs);
    for (size_t i = 0; i < lphi.size(); ++i) lphi[i] = log(1.0 + Phi[i]);   // src/misc.jl:53
    int rc;
    const long long ns = n - n1 + 1;
    if ((rc = h->d_s_in.ensure(s32.size() * 4)) || (rc = h->d_order.ensure(o32.size() * 4)) ||
        (rc = h->d_Pi.ensure((size_t)C * K * N * 8)) || (rc = h->d_logphi.ensure(lphi.size() * 8)) ||
        (rc = h->d_s_out.ensure(s32.size() * 4)) || (rc = h->d_lw.ensure((size_t)C * P * 8)))
        return rc;
    if (feature_flag && (rc = h->d_flags.ensure((size_t)C * h->sumD))) return rc;
    if (trace && (rc = h->d_trace.ensure((size_t)C * ns * (2 + 2 * K) * 8))) return rc;
    HIP_TRY(hipMemcpyAsync(h->d_s_in.p, s32.data(), s32.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->d_order.p, o32.data(), o32.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->d_Pi.p, Pi, (size_t)C * K * N * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->d_logphi.p, lphi.data(), lphi.size() * 8, hipMemcpyHostToDevice, h->stream));
    if (feature_flag) HIP_TRY(hipMemcpyAsync(h->d_flags.p, feature_flag, (size_t)C * h->sumD, hipMemcpyHostToDevice, h->stream));

    SweepArgs a;
    fill_sweep_call(h, a, iter, n1, lw_init, (const int *)h->d_s_in.p, (const int *)h->d_order.p, (const double *)h->d_Pi.p,
                    (const double *)h->d_logphi.p, feature_flag ? (const unsigned char *)h->d_flags.p : nullptr, (int *)h->d_s_out.p,
                    (double *)h->d_lw.p, nullptr, nullptr, nullptr, trace ? (double *)h->d_trace.p : nullptr);
    if ((rc = launch_sweep_groups(h, a, h->stream))) return rc;
    std::vector<int> so(s32.size()), ps(C), er(C);
    std::vector<long long> stv((size_t)C * 8);
    HIP_TRY(hipMemcpyAsync(so.data(), h->d_s_out.p, so.size() * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(ps.data(), h->d_pstar.p, (size_t)C * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(er.data(), h->d_err.p, (size_t)C * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(stv.data(), h->d_stats.p, stv.size() * 8, hipMemcpyDeviceToHost, h->stream));
    if (logweight) HIP_TRY(hipMemcpyAsync(logweight, h->d_lw.p, (size_t)C * P * 8, hipMemcpyDeviceToHost, h->stream));
    if (trace) HIP_TRY(hipMemcpyAsync(trace, h->d_trace.p, (size_t)C * ns * (2 + 2 * K) * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->swept = true; h->last_n1 = n1;
    for (int c = 0; c < C; ++c)
        if (er[c] != 0)
            return fail(er[c] == PMDI_E_POOL ? PMDI_E_POOL : PMDI_E_STATE,
                        er[c] == PMDI_E_POOL ? "chain %d: cluster pool capacity %lld exceeded" : "chain %d: kernel reported error", c, h->cap);
    if (s_out) for (size_t i = 0; i < so.size(); ++i) s_out[i] = (int64_t)so[i] + 1;
    if (p_star) for (int c = 0; c < C; ++c) p_star[c] = (int64_t)ps[c] + 1;
    if (stats)
        for (int c = 0; c < C; ++c) {
            memset(&stats[c], 0, sizeof(pmdi_sweep_stats));
            stats[c].n_operations = stv[(size_t)c * 8 + ST_NOPS];
            stats[c].n_resamples = stv[(size_t)c * 8 + ST_NRESAMPLE];
            stats[c].n_clones = stv[(size_t)c * 8 + ST_NCLONES];
            stats[c].max_id = stv[(size_t)c * 8 + ST_MAXID];
            stats[c].sum_classes = stv[(size_t)c * 8 + ST_SUMCLASSES];
            stats[c].steps_fast = stv[(size_t)c * 8 + 5];
            stats[c].steps_converted = stv[(size_t)c * 8 + 6];
            stats[c].steps_fallback = stv[(size_t)c * 8 + 7];
        }
    return PMDI_OK;
}

int pmdi_export_state(pmdi_handle *h, int32_t chain, int64_t *particle, int64_t *counts, int64_t *cluster_n,
                      int64_t *max_id)
{
    if (!h) return fail(PMDI_E_ARG, "null handle");
    if (!h->swept) return fail(PMDI_E_STATE, "no sweep has run on this handle");
    if (chain < 0 || chain >= h->cfg.n_chains) return fail(PMDI_E_ARG, "chain out of range");
    const int K = h->cfg.K, N = h->cfg.N, P = h->cfg.P;
    const long long cap = h->cap;
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    std::vector<int> ks((size_t)PMDI_KMAX_I * 2);
    HIP_TRY(hipMemcpy(ks.data(), (char *)h->d_kstate.p + (size_t)chain * PMDI_KMAX_I * 2 * 4, ks.size() * 4, hipMemcpyDeviceToHost));
    std::vector<int> tmp((size_t)N * P), tc((size_t)cap + 1), col((size_t)P);
    for (int k = 0; k < K; ++k) {
        const DsetDev &d = h->ds[k];
        const char *base = d.arena + (size_t)chain * d.stride;
        const int cur = ks[(size_t)k * 2 + 1];
        if (particle) {
            // the device keeps the distinct columns of particle[:, :, k] and a column index per particle
            HIP_TRY(hipMemcpy(tmp.data(), base + d.o_particle[cur], tmp.size() * 4, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(col.data(), base + d.o_col, col.size() * 4, hipMemcpyDeviceToHost));
            for (int p = 0; p < P; ++p) {                             // particle[n, p, k], column-major
                if (col[p] < 0 || col[p] >= P) return fail(PMDI_E_STATE, "corrupt column index %d of particle %d", col[p], p);
                for (int nn = 0; nn < N; ++nn) particle[((size_t)k * P + p) * N + nn] = tmp[(size_t)col[p] * N + nn];
            }
        }
        if (counts) {
            HIP_TRY(hipMemcpy(tc.data(), base + d.o_counts, tc.size() * 4, hipMemcpyDeviceToHost));
            for (long long id = 1; id <= cap; ++id) counts[(size_t)k * cap + (id - 1)] = tc[id];
        }
        if (cluster_n) {
            HIP_TRY(hipMemcpy(tc.data(), base + d.o_cn, tc.size() * 4, hipMemcpyDeviceToHost));
            for (long long id = 1; id <= cap; ++id) cluster_n[(size_t)k * cap + (id - 1)] = tc[id];
        }
        if (max_id) max_id[k] = ks[(size_t)k * 2];
    }
    return PMDI_OK;
}

int pmdi_feature_select(pmdi_handle *h, int64_t iter, const int64_t *s_traj, uint8_t *feature_flag, double *feature_prob)
{
    if (!h || !s_traj) return fail(PMDI_E_ARG, "null argument");
    const int K = h->cfg.K, N = h->cfg.N, C = h->cfg.n_chains;
    const long long n = h->cfg.n;
    HIP_TRY(hipSetDevice(h->cfg.device));
    std::vector<int> t32((size_t)C * K * n);
    for (size_t i = 0; i < t32.size(); ++i) {
        const long long v = s_traj[i];
        if (v < 1 || v > N) return fail(PMDI_E_DATA, "s_traj[%zu]=%lld outside 1..N", i, v);
        t32[i] = (int)(v - 1);
    }
    HIP_TRY(hipMemcpyAsync(h->d_traj.p, t32.data(), t32.size() * 4, hipMemcpyHostToDevice, h->stream));
    FeatSelArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.K = K; fa.N = N; fa.sumD = h->sumD; fa.n = n; fa.iter = (unsigned)iter; fa.seed = h->cfg.seed;
    for (int k = 0; k < K; ++k) fa.ds[k] = h->ds[k];
    fa.traj = (const int *)h->d_traj.p; fa.lm = (double *)h->d_lm.p; fa.firstpos = (int *)h->d_firstpos.p;
    fa.fnull = (const double *)h->d_fnull.p; fa.flags_out = (unsigned char *)h->d_fflags.p; fa.prob_out = (double *)h->d_fprob.p;
    hipError_t e = pmdi_launch_featsel(fa, C, h->stream);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "feature-select launch: %s", hipGetErrorString(e));
    if (feature_flag) HIP_TRY(hipMemcpyAsync(feature_flag, h->d_fflags.p, (size_t)C * h->sumD, hipMemcpyDeviceToHost, h->stream));
    if (feature_prob) HIP_TRY(hipMemcpyAsync(feature_prob, h->d_fprob.p, (size_t)C * h->sumD * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return PMDI_OK;
}

// ---- stand-alone cluster batches ------------------------------------------
int pmdi_clusters_new(pmdi_handle *h, int32_t k, int32_t B, pmdi_cluster_batch **out)
{
    if (!h || !out) return fail(PMDI_E_ARG, "null argument");
    *out = nullptr;
    if (k < 0 || k >= h->cfg.K || B < 1) return fail(PMDI_E_ARG, "bad dataset index or batch size");
    HIP_TRY(hipSetDevice(h->cfg.device));
    pmdi_cluster_batch *cb = new (std::nothrow) pmdi_cluster_batch();
    if (!cb) return fail(PMDI_E_MEMORY, "out of host memory");
    cb->h = h; cb->k = k; cb->B = B;
    cb->d = h->ds[k];
    h->children += 1;
    cb->d.stride = layout_arena(cb->d, h->cfg.N, h->cfg.P, B, 0, false);
    hipError_t e = hipMalloc(&cb->arena, cb->d.stride);
    if (e != hipSuccess) { h->children -= 1; delete cb; return fail(PMDI_E_MEMORY, "hipMalloc: %s", hipGetErrorString(e)); }
    cb->d.arena = (char *)cb->arena;
    (void)hipMemset(cb->arena, 0, cb->d.stride);
    if (cb->d.kind == K_GAUSSIAN) {     // GaussianCluster(dataFile): mu=Sigma=0, lambda=1, beta=0.5 (gaussian_cluster.jl:17-21)
        std::vector<double> ml((size_t)(B + 1) * cb->d.D * 2), sb(ml.size());
        for (size_t i = 0; i < ml.size(); i += 2) { ml[i] = 0.0; ml[i + 1] = 1.0; sb[i] = 0.0; sb[i + 1] = 0.5; }
        (void)hipMemcpy(cb->d.arena + cb->d.o_ml, ml.data(), ml.size() * 8, hipMemcpyHostToDevice);
        (void)hipMemcpy(cb->d.arena + cb->d.o_sb, sb.data(), sb.size() * 8, hipMemcpyHostToDevice);
    }
    *out = cb;
    return PMDI_OK;
}

int pmdi_clusters_free(pmdi_cluster_batch *cb)
{
    if (!cb) return PMDI_OK;
    (void)hipSetDevice(cb->h->cfg.device);
    if (cb->arena) (void)hipFree(cb->arena);
    if (cb->h->children > 0) cb->h->children -= 1;
    delete cb;                  // (and its DevBufs)
    return PMDI_OK;
}

static int batch_args(pmdi_cluster_batch *cb, const int64_t *rows, const uint8_t *flag, ClusterBatchArgs &a)
{
    const long long n = cb->h->cfg.n;
    int rc;
    memset(&a, 0, sizeof(a));
    a.ds = cb->d; a.B = cb->B;
    if (rows) {
        std::vector<int> r32(cb->B);
        for (int b = 0; b < cb->B; ++b) {
            if (rows[b] < 1 || rows[b] > n) return fail(PMDI_E_ARG, "row %lld outside 1..n", (long long)rows[b]);
            r32[b] = (int)(rows[b] - 1);
        }
        if ((rc = cb->d_rows.ensure((size_t)cb->B * 4))) return rc;
        HIP_TRY(hipMemcpy(cb->d_rows.p, r32.data(), (size_t)cb->B * 4, hipMemcpyHostToDevice));
        a.rows = (const int *)cb->d_rows.p;
    }
    if (flag) {
        if ((rc = cb->d_flags.ensure((size_t)cb->d.D))) return rc;
        HIP_TRY(hipMemcpy(cb->d_flags.p, flag, (size_t)cb->d.D, hipMemcpyHostToDevice));
        a.flags = (const unsigned char *)cb->d_flags.p;
    }
    return 0;
}

int pmdi_cluster_add(pmdi_cluster_batch *cb, const int64_t *rows, const uint8_t *feature_flag)
{
    if (!cb || !rows) return fail(PMDI_E_ARG, "null argument");
    HIP_TRY(hipSetDevice(cb->h->cfg.device));
    ClusterBatchArgs a;
    int rc = batch_args(cb, rows, feature_flag, a);
    if (rc) return rc;
    hipError_t e = pmdi_launch_cluster_add(a, cb->h->stream);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "cluster_add launch: %s", hipGetErrorString(e));
    HIP_TRY(hipStreamSynchronize(cb->h->stream));
    return PMDI_OK;
}

int pmdi_calc_logprob(pmdi_cluster_batch *cb, const int64_t *obs_rows, const uint8_t *feature_flag, double *out)
{
    if (!cb || !obs_rows || !out) return fail(PMDI_E_ARG, "null argument");
    HIP_TRY(hipSetDevice(cb->h->cfg.device));
    ClusterBatchArgs a;
    int rc = batch_args(cb, obs_rows, feature_flag, a);
    if (rc) return rc;
    if ((rc = cb->d_out.ensure((size_t)cb->B * 8))) return rc;
    a.out = (double *)cb->d_out.p;
    hipError_t e = pmdi_launch_cluster_logprob(a, cb->h->stream);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "calc_logprob launch: %s", hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(out, cb->d_out.p, (size_t)cb->B * 8, hipMemcpyDeviceToHost, cb->h->stream));
    HIP_TRY(hipStreamSynchronize(cb->h->stream));
    return PMDI_OK;
}

int pmdi_calc_logmarginal(pmdi_cluster_batch *cb, double *out)
{
    if (!cb || !out) return fail(PMDI_E_ARG, "null argument");
    HIP_TRY(hipSetDevice(cb->h->cfg.device));
    ClusterBatchArgs a;
    int rc = batch_args(cb, nullptr, nullptr, a);
    if (rc) return rc;
    const size_t bytes = (size_t)cb->B * cb->d.D * 8;
    if ((rc = cb->d_out.ensure(bytes))) return rc;
    a.out = (double *)cb->d_out.p;
    hipError_t e = pmdi_launch_cluster_logmarginal(a, cb->h->stream);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "calc_logmarginal launch: %s", hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(out, cb->d_out.p, bytes, hipMemcpyDeviceToHost, cb->h->stream));
    HIP_TRY(hipStreamSynchronize(cb->h->stream));
    return PMDI_OK;
}

int pmdi_cluster_stats(pmdi_cluster_batch *cb, double *out, int64_t *stride)
{
    if (!cb || !stride) return fail(PMDI_E_ARG, "null argument");
    const DsetDev &d = cb->d;
    const int D = d.D, B = cb->B;
    const int64_t st = 1 + (d.kind == K_GAUSSIAN ? 4 * (int64_t)D : d.kind == K_CATEGORICAL ? (int64_t)D * d.L : (int64_t)D);
    *stride = st;
    if (!out) return PMDI_OK;
    HIP_TRY(hipSetDevice(cb->h->cfg.device));
    HIP_TRY(hipStreamSynchronize(cb->h->stream));
    std::vector<int> cn((size_t)B + 1);
    HIP_TRY(hipMemcpy(cn.data(), d.arena + d.o_cn, cn.size() * 4, hipMemcpyDeviceToHost));
    if (d.kind == K_GAUSSIAN) {
        std::vector<double> ml((size_t)(B + 1) * D * 2), sb(ml.size());
        HIP_TRY(hipMemcpy(ml.data(), d.arena + d.o_ml, ml.size() * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(sb.data(), d.arena + d.o_sb, sb.size() * 8, hipMemcpyDeviceToHost));
        for (int b = 0; b < B; ++b) {
            double *o = out + (size_t)b * st;
            o[0] = cn[b + 1];
            for (int q = 0; q < D; ++q) {
                const size_t e = ((size_t)(b + 1) * D + q) * 2;
                o[1 + q] = ml[e]; o[1 + D + q] = sb[e]; o[1 + 2 * D + q] = ml[e + 1]; o[1 + 3 * D + q] = sb[e + 1];
            }
        }
    } else if (d.kind == K_CATEGORICAL) {
        std::vector<int> c((size_t)(B + 1) * D * d.L);
        HIP_TRY(hipMemcpy(c.data(), d.arena + d.o_cnt, c.size() * 4, hipMemcpyDeviceToHost));
        for (int b = 0; b < B; ++b) {
            double *o = out + (size_t)b * st;
            o[0] = cn[b + 1];
            for (int q = 0; q < D; ++q)
                for (int l = 0; l < d.L; ++l) o[1 + (size_t)q * d.L + l] = c[((size_t)(b + 1) * D + q) * d.L + l];
        }
    } else {
        std::vector<long long> s((size_t)(B + 1) * D);
        HIP_TRY(hipMemcpy(s.data(), d.arena + d.o_nbs, s.size() * 8, hipMemcpyDeviceToHost));
        for (int b = 0; b < B; ++b) {
            double *o = out + (size_t)b * st;
            o[0] = cn[b + 1];
            for (int q = 0; q < D; ++q) o[1 + q] = (double)s[(size_t)(b + 1) * D + q];
        }
    }
    return PMDI_OK;
}

}  // extern "C"

// ---- device-resident Gibbs chains ---------------------------------------------------------------
namespace {
template <class Tp>
int galloc(pmdi_gibbs *g, Tp **p, size_t count)
{
    void *q = nullptr;
    size_t bytes = count * sizeof(Tp);
    if (bytes == 0) bytes = 16;
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) { *p = nullptr; return fail(PMDI_E_MEMORY, "hipMalloc(%zu bytes): %s", bytes, hipGetErrorString(e)); }
    g->owned.push_back(q);
    *p = (Tp *)q;
    return 0;
}
}  // namespace

extern "C" {

int pmdi_gibbs_destroy(pmdi_gibbs *g)
{
    if (!g) return PMDI_OK;
    (void)hipSetDevice(g->device);
    (void)hipDeviceSynchronize();
    for (void *p : g->owned) (void)hipFree(p);
    if (g->h && g->h->children > 0) g->h->children -= 1;      // (the handle outlives its children: pmdi_destroy refuses otherwise)
    delete g;
    return PMDI_OK;
}

int pmdi_gibbs_create(pmdi_handle *h, double rho, int32_t feature_select, pmdi_gibbs **out)
{
    if (!h || !out) return fail(PMDI_E_ARG, "null argument");
    *out = nullptr;
    if (!(rho < 1.0 && rho > 0.0)) return fail(PMDI_E_ARG, "rho must be between 0 and 1");          // src/pmdi.jl:53
    const int K = h->cfg.K, N = h->cfg.N, P = h->cfg.P, C = h->cfg.n_chains;
    const long long n = h->cfg.n;
    const long long n1 = (long long)floor(rho * (double)n);                                           // :161
    if (n1 < 1) return fail(PMDI_E_ARG, "floor(rho*n) = %lld < 1 (the reference indexes order_obs[0], SURVEY Q8)", n1);
    HIP_TRY(hipSetDevice(h->cfg.device));
    pmdi_gibbs *g = new (std::nothrow) pmdi_gibbs();
    if (!g) return fail(PMDI_E_MEMORY, "out of host memory");
    g->h = h; g->device = h->cfg.device; g->n1 = n1; g->feature_select = feature_select ? 1 : 0;
    h->children += 1;
    GibbsArgs &a = g->ga;
    a.K = K; a.N = N; a.npairs = h->npairs; a.n_chains = C; a.n = n; a.iter = 0; a.seed = h->cfg.seed;
    int rc = 0;
    double *lg = nullptr;
    const size_t tabsz = (size_t)K * K * N * N;
    if ((rc = galloc(g, &a.M, (size_t)C * K)) || (rc = galloc(g, &a.gamma, (size_t)C * K * N)) ||
        (rc = galloc(g, &a.gamma0, (size_t)C * K * N)) || (rc = galloc(g, &a.Phi, (size_t)C * h->npairs)) ||
        (rc = galloc(g, &a.vZ, (size_t)C * 2)) || (rc = galloc(g, &a.s, (size_t)C * K * n)) ||
        (rc = galloc(g, &g->s_next, (size_t)C * K * n)) || (rc = galloc(g, &a.order, (size_t)C * n)) ||
        (rc = galloc(g, &a.Pi, (size_t)C * K * N)) || (rc = galloc(g, &a.logphi, (size_t)C * h->npairs)) ||
        (rc = galloc(g, &a.wscr, (size_t)C * (n + 1))) || (rc = galloc(g, &lg, (size_t)n + 3)) ||
        (rc = galloc(g, &g->flags, (size_t)C * h->sumD)) || (rc = galloc(g, &g->fprob, (size_t)C * h->sumD)) ||
        (rc = galloc(g, &g->lw, (size_t)C * P)) || (rc = galloc(g, &g->pstar, (size_t)C)) ||
        (rc = galloc(g, &g->stats, (size_t)C * 8)) || (rc = galloc(g, &g->err, (size_t)C))) {
        pmdi_gibbs_destroy(g);
        return rc;
    }
    a.ctab_lds = (tabsz * 4 <= 96 * 1024) ? 1 : 0;
    a.order_lds = ((size_t)n * 4 <= 96 * 1024) ? 1 : 0;
    a.ctab = nullptr;
    if (!a.ctab_lds && K > 1 && (rc = galloc(g, &a.ctab, (size_t)C * tabsz))) { pmdi_gibbs_destroy(g); return rc; }
    {
        std::vector<double> t((size_t)n + 3);
        for (size_t m = 0; m < t.size(); ++m) t[m] = lgamma((double)m);          // t[0] = inf is never read
        if (hipMemcpy(lg, t.data(), t.size() * 8, hipMemcpyHostToDevice) != hipSuccess) { pmdi_gibbs_destroy(g); return fail(PMDI_E_DEVICE, "memcpy failed"); }
        a.lgtab = lg;
    }
    // featureFlag (src/pmdi.jl:106-110): rand(Bool) per feature when feature selection is on, else all true
    {
        std::vector<unsigned char> fl((size_t)C * h->sumD, 1);
        if (g->feature_select)
            for (int c = 0; c < C; ++c)
                for (int k = 0; k < K; ++k)
                    for (int q = 0; q < h->ds[k].D; ++q)
                        fl[(size_t)c * h->sumD + h->ds[k].flag_off + q] =
                            pmdi_arith::uniform01(h->cfg.seed + (unsigned long long)c, 0, 0, (unsigned)k, (unsigned)q, SITE_INIT_FLAGS) < 0.5 ? 1 : 0;
        if (hipMemcpy(g->flags, fl.data(), fl.size(), hipMemcpyHostToDevice) != hipSuccess) { pmdi_gibbs_destroy(g); return fail(PMDI_E_DEVICE, "memcpy failed"); }
    }
    if (hipMemset(g->err, 0, (size_t)C * 4) != hipSuccess || hipMemset(g->stats, 0, (size_t)C * 64) != hipSuccess ||
        hipMemset(g->s_next, 0, (size_t)C * K * n * 4) != hipSuccess) {
        pmdi_gibbs_destroy(g);
        return fail(PMDI_E_DEVICE, "memset failed");
    }
    hipError_t e = pmdi_launch_gibbs_init(a, h->stream);
    if (e != hipSuccess) { pmdi_gibbs_destroy(g); return fail(PMDI_E_DEVICE, "gibbs init launch: %s", hipGetErrorString(e)); }
    if (hipStreamSynchronize(h->stream) != hipSuccess) { pmdi_gibbs_destroy(g); return fail(PMDI_E_DEVICE, "gibbs init kernel failed"); }
    *out = g;
    return PMDI_OK;
}

int pmdi_gibbs_step(pmdi_gibbs *g, int32_t what, void *stream)
{
    if (!g) return fail(PMDI_E_ARG, "null argument");
    pmdi_handle *h = g->h;
    HIP_TRY(hipSetDevice(h->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    GibbsArgs a = g->ga;
    hipError_t e;
    switch (what) {
    case PMDI_STEP_BEGIN:
        g->iter += 1;
        return PMDI_OK;
    case PMDI_STEP_HYPERS:
        a.iter = (unsigned)g->iter;
        e = pmdi_launch_hypers(a, 1, st);
        if (e != hipSuccess) return fail(PMDI_E_DEVICE, "hypers launch: %s", hipGetErrorString(e));
        return PMDI_OK;
    case PMDI_STEP_SWEEP: {
        // the first error of a chain sticks (a later, successful sweep does not reset it): pmdi_gibbs_results reports it,
        // pmdi_gibbs_set of that chain clears it.  A failed chain keeps its allocations (the kernel copies s_in to s_out).
        h->err_keep = 1;
        const int rc = pmdi_sweep_device(h, g->iter, a.s, a.order, g->n1, a.Pi, a.logphi, g->flags, g->iter == 1 ? 0.0 : 1.0,
                                         g->s_next, g->lw, g->pstar, (int64_t *)g->stats, g->err, stream);
        h->err_keep = 0;
        if (rc) return rc;
        std::swap(g->ga.s, g->s_next);               // s = sstar[p_star, :, :] (src/pmdi.jl:373)
        return PMDI_OK;
    }
    case PMDI_STEP_FEATSEL: {
        FeatSelArgs fa;
        memset(&fa, 0, sizeof(fa));
        fa.K = h->cfg.K; fa.N = h->cfg.N; fa.sumD = h->sumD; fa.n = h->cfg.n; fa.iter = (unsigned)g->iter; fa.seed = h->cfg.seed;
        for (int k = 0; k < h->cfg.K; ++k) fa.ds[k] = h->ds[k];
        fa.traj = a.s; fa.lm = (double *)h->d_lm.p; fa.firstpos = (int *)h->d_firstpos.p;
        fa.fnull = (const double *)h->d_fnull.p; fa.flags_out = g->flags; fa.prob_out = g->fprob;
        e = pmdi_launch_featsel(fa, h->cfg.n_chains, st);
        if (e != hipSuccess) return fail(PMDI_E_DEVICE, "feature-select launch: %s", hipGetErrorString(e));
        return PMDI_OK;
    }
    case PMDI_STEP_ALIGN:
        a.iter = (unsigned)g->iter;
        e = pmdi_launch_align(a, st);
        if (e != hipSuccess) return fail(PMDI_E_DEVICE, "align launch: %s", hipGetErrorString(e));
        return PMDI_OK;
    default:
        return fail(PMDI_E_ARG, "unknown step %d", what);
    }
}

int pmdi_gibbs_iterate(pmdi_gibbs *g, int64_t n_iter, uint8_t *samples, void *stream)
{
    if (!g || n_iter < 0) return fail(PMDI_E_ARG, "bad argument");
    const pmdi_handle *h = g->h;
    const long long per = (long long)h->cfg.n_chains * h->cfg.K * h->cfg.n;
    for (int64_t t = 0; t < n_iter; ++t) {
        int rc;
        if ((rc = pmdi_gibbs_step(g, PMDI_STEP_BEGIN, stream)) || (rc = pmdi_gibbs_step(g, PMDI_STEP_HYPERS, stream)) ||
            (rc = pmdi_gibbs_step(g, PMDI_STEP_SWEEP, stream)))
            return rc;
        if (g->feature_select && (rc = pmdi_gibbs_step(g, PMDI_STEP_FEATSEL, stream))) return rc;
        if ((rc = pmdi_gibbs_step(g, PMDI_STEP_ALIGN, stream))) return rc;
        if (samples) {
            hipError_t e = pmdi_launch_pack_samples(g->ga.s, samples + (size_t)t * per, per, (hipStream_t)stream);
            if (e != hipSuccess) return fail(PMDI_E_DEVICE, "pack-samples launch: %s", hipGetErrorString(e));
        }
    }
    return PMDI_OK;
}

int64_t pmdi_gibbs_iterations(const pmdi_gibbs *g) { return g ? g->iter : 0; }

int pmdi_gibbs_pack_samples(pmdi_gibbs *g, uint8_t *out, void *stream)
{
    if (!g || !out) return fail(PMDI_E_ARG, "null argument");
    const pmdi_handle *h = g->h;
    HIP_TRY(hipSetDevice(h->cfg.device));
    hipError_t e = pmdi_launch_pack_samples(g->ga.s, out, (long long)h->cfg.n_chains * h->cfg.K * h->cfg.n, (hipStream_t)stream);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "pack-samples launch: %s", hipGetErrorString(e));
    return PMDI_OK;
}

int pmdi_gibbs_device_view(pmdi_gibbs *g, pmdi_gibbs_view *v)
{
    if (!g || !v) return fail(PMDI_E_ARG, "null argument");
    v->M = g->ga.M; v->gamma = g->ga.gamma; v->gamma0 = g->ga.gamma0; v->Phi = g->ga.Phi; v->vZ = g->ga.vZ;
    v->s = g->ga.s; v->order_obs = g->ga.order; v->Pi = g->ga.Pi; v->log1p_phi = g->ga.logphi;
    v->feature_flag = g->flags; v->feature_prob = g->fprob; v->logweight = g->lw; v->p_star = g->pstar;
    v->stats = (int64_t *)g->stats; v->err = g->err; v->n1 = g->n1;
    return PMDI_OK;
}

int pmdi_gibbs_get(pmdi_gibbs *g, int32_t chain, double *M, double *gamma, double *gamma0, double *Phi, double *vZ,
                   int64_t *s, int64_t *order_obs, uint8_t *feature_flag)
{
    if (!g) return fail(PMDI_E_ARG, "null argument");
    const pmdi_handle *h = g->h;
    const int K = h->cfg.K, N = h->cfg.N;
    const long long n = h->cfg.n;
    if (chain < 0 || chain >= h->cfg.n_chains) return fail(PMDI_E_ARG, "chain out of range");
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(hipDeviceSynchronize());
    const GibbsArgs &a = g->ga;
    if (M) HIP_TRY(hipMemcpy(M, a.M + (size_t)chain * K, (size_t)K * 8, hipMemcpyDeviceToHost));
    if (gamma) HIP_TRY(hipMemcpy(gamma, a.gamma + (size_t)chain * K * N, (size_t)K * N * 8, hipMemcpyDeviceToHost));    // N x K column-major
    if (gamma0) HIP_TRY(hipMemcpy(gamma0, a.gamma0 + (size_t)chain * K * N, (size_t)K * N * 8, hipMemcpyDeviceToHost));
    if (Phi) HIP_TRY(hipMemcpy(Phi, a.Phi + (size_t)chain * h->npairs, (size_t)h->npairs * 8, hipMemcpyDeviceToHost));
    if (vZ) HIP_TRY(hipMemcpy(vZ, a.vZ + (size_t)chain * 2, 16, hipMemcpyDeviceToHost));
    if (s) {
        std::vector<int> t((size_t)K * n);
        HIP_TRY(hipMemcpy(t.data(), a.s + (size_t)chain * K * n, t.size() * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < t.size(); ++i) s[i] = (int64_t)t[i] + 1;         // n x K column-major, labels 1..N
    }
    if (order_obs) {
        std::vector<int> t((size_t)n);
        HIP_TRY(hipMemcpy(t.data(), a.order + (size_t)chain * n, t.size() * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < t.size(); ++i) order_obs[i] = (int64_t)t[i] + 1;
    }
    if (feature_flag) HIP_TRY(hipMemcpy(feature_flag, g->flags + (size_t)chain * h->sumD, (size_t)h->sumD, hipMemcpyDeviceToHost));
    return PMDI_OK;
}

int pmdi_gibbs_set(pmdi_gibbs *g, int32_t chain, const double *M, const double *gamma, const double *gamma0, const double *Phi,
                   const double *vZ, const int64_t *s, const int64_t *order_obs, const uint8_t *feature_flag)
{
    if (!g) return fail(PMDI_E_ARG, "null argument");
    const pmdi_handle *h = g->h;
    const int K = h->cfg.K, N = h->cfg.N;
    const long long n = h->cfg.n;
    if (chain < 0 || chain >= h->cfg.n_chains) return fail(PMDI_E_ARG, "chain out of range");
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(hipDeviceSynchronize());
    const GibbsArgs &a = g->ga;
    if (M) HIP_TRY(hipMemcpy(a.M + (size_t)chain * K, M, (size_t)K * 8, hipMemcpyHostToDevice));
    if (gamma) HIP_TRY(hipMemcpy(a.gamma + (size_t)chain * K * N, gamma, (size_t)K * N * 8, hipMemcpyHostToDevice));
    if (gamma0) HIP_TRY(hipMemcpy(a.gamma0 + (size_t)chain * K * N, gamma0, (size_t)K * N * 8, hipMemcpyHostToDevice));
    if (Phi) HIP_TRY(hipMemcpy(a.Phi + (size_t)chain * h->npairs, Phi, (size_t)h->npairs * 8, hipMemcpyHostToDevice));
    if (vZ) HIP_TRY(hipMemcpy(a.vZ + (size_t)chain * 2, vZ, 16, hipMemcpyHostToDevice));
    if (s) {
        std::vector<int> t((size_t)K * n);
        for (size_t i = 0; i < t.size(); ++i) {
            if (s[i] < 1 || s[i] > N) return fail(PMDI_E_DATA, "s[%zu]=%lld outside 1..N", i, (long long)s[i]);
            t[i] = (int)(s[i] - 1);
        }
        HIP_TRY(hipMemcpy(a.s + (size_t)chain * K * n, t.data(), t.size() * 4, hipMemcpyHostToDevice));
    }
    if (order_obs) {
        std::vector<int> t((size_t)n);
        for (size_t i = 0; i < t.size(); ++i) {
            if (order_obs[i] < 1 || order_obs[i] > n) return fail(PMDI_E_DATA, "order_obs[%zu]=%lld outside 1..n", i, (long long)order_obs[i]);
            t[i] = (int)(order_obs[i] - 1);
        }
        HIP_TRY(hipMemcpy(a.order + (size_t)chain * n, t.data(), t.size() * 4, hipMemcpyHostToDevice));
    }
    if (feature_flag) HIP_TRY(hipMemcpy(g->flags + (size_t)chain * h->sumD, feature_flag, (size_t)h->sumD, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(g->err + chain, 0, 4));                 // a chain given a new state starts without its sticky error
    return PMDI_OK;
}

int pmdi_gibbs_results(pmdi_gibbs *g, int64_t *stats, int32_t *err, int64_t *p_star, double *logweight)
{
    if (!g) return fail(PMDI_E_ARG, "null argument");
    const pmdi_handle *h = g->h;
    const int C = h->cfg.n_chains;
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(hipDeviceSynchronize());
    if (stats) HIP_TRY(hipMemcpy(stats, g->stats, (size_t)C * 64, hipMemcpyDeviceToHost));
    std::vector<int> er(C);
    HIP_TRY(hipMemcpy(er.data(), g->err, (size_t)C * 4, hipMemcpyDeviceToHost));
    if (err) memcpy(err, er.data(), (size_t)C * 4);
    if (p_star) {
        std::vector<int> ps(C);
        HIP_TRY(hipMemcpy(ps.data(), g->pstar, (size_t)C * 4, hipMemcpyDeviceToHost));
        for (int c = 0; c < C; ++c) p_star[c] = (int64_t)ps[c] + 1;
    }
    if (logweight) HIP_TRY(hipMemcpy(logweight, g->lw, (size_t)C * h->cfg.P * 8, hipMemcpyDeviceToHost));
    for (int c = 0; c < C; ++c)
        if (er[c] != 0)
            return fail(er[c] == PMDI_E_POOL ? PMDI_E_POOL : PMDI_E_STATE,
                        er[c] == PMDI_E_POOL ? "chain %d: cluster pool capacity %lld exceeded" : "chain %d: kernel reported error", c, h->cap);
    return PMDI_OK;
}

}  // extern "C"
