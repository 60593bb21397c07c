// pmdi_sweep_carve.h -- the LDS layout of the general sweep kernel (pmdi_sweep_body.h): byte offsets of its arrays as a function of
// the argument block, shared by the kernel and the host's sizing.  A plain header: the launch planner (pmdi_plan.cpp) compiles it
// with any C++ compiler.
#pragma once
#include "pmdi_internal.h"

namespace {

// ---------------------------------------------------------------------------
struct Carve {  // byte offsets of the LDS arrays (shared by host sizing and the kernel)
    size_t xs, pis, lw, term, lpl, cdf, scan, red, pid, sid, kv, lead_of, slot_of, cl_lead, cl_val,
        need, need_slot, item_id, dl, dl_slot, h1k, h1a, h2k, h2a, h2b, ktab_minp, ktab_val, klist, kl_v, wk,
        kl_key, fl_p, fl_slot, fl_nnew, fl_tgt, bm_fresh, bm_clone, bm_keep, bm_reuse, col, kncol, leaf_i1, leaf_n, leaf_tot, leaf_carry, leaf_prog, kmaxid, kncls, kcur, knflag, khint, misc, ph, stat,
        fl, news, total;
};

__host__ __device__ inline void carve_lds(const SweepArgs &a, Carve &c)
{
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o = (o + bytes + 15) & ~(size_t)15; return at; };
    const int Dp = (a.Dmax + 15) & ~15;
    // ---- fixed-size tables: compile-time offsets ----
    c.scan = take(16 * 8);
    c.red = take(48 * 8);
    c.misc = take(16 * 4);
    c.ph = take(16 * 8);
#ifdef PMDI_RESAMPLE_TIMERS
    c.stat = take(24 * 8);
#else
    c.stat = take(8 * 8);
#endif
    c.wk = take(PMDI_KMAX_I * 8 * 8);
    c.kmaxid = take(PMDI_KMAX_I * 4);
    c.kncls = take(PMDI_KMAX_I * 4);
    c.kcur = take(PMDI_KMAX_I * 4);
    c.knflag = take(PMDI_KMAX_I * 4);
    c.khint = take(PMDI_KMAX_I * 4);
    c.kncol = take(PMDI_KMAX_I * 4);
    c.leaf_i1 = take(64 * 4);
    c.leaf_n = take(64 * 4);
    c.leaf_tot = take(64 * 8);
    c.leaf_carry = take(64 * 8);
    c.leaf_prog = take(256);
    c.dl_slot = take((size_t)PMDI_DL_LDS * 4);
    c.h1k = take((size_t)PMDI_HT_SIZE * 4);
    c.h1a = take((size_t)PMDI_HT_SIZE * 4);
    c.h2k = take((size_t)PMDI_HT_SIZE * 4);
    c.h2a = take((size_t)PMDI_HT_SIZE * 4);
    c.h2b = take((size_t)PMDI_HT_SIZE * 4);
    c.fl_p = take((size_t)PMDI_HT_SIZE * 4);
    c.fl_slot = take((size_t)PMDI_HT_SIZE * 4);
    c.fl_nnew = take((size_t)PMDI_HT_SIZE * 4);
    c.fl_tgt = take((size_t)PMDI_HT_SIZE * 4);
    // ---- tables of (class, label) items: a.item_cap entries each (256, or 384 when N > 32 so that more than
    // five classes stay on the fast path); need .. dl are contiguous (the fallback step's cluster list) ----
    const size_t icap = (size_t)a.item_cap;
    const int KL = a.ksplit ? 1 : a.K;                       // datasets this workgroup sweeps
    c.lpl = take(icap * 8);
    c.cdf = take((2 * icap + 4) * 8);                        // rows of N + 2: CDF, log-increment, one-hot label
    c.need = take(icap * 4);
    c.need_slot = take(icap * 4);
    c.item_id = take(icap * 4);
    c.ktab_minp = take(icap * 4);
    c.ktab_val = take(icap * 4);
    c.klist = take(icap * 4);
    c.kl_v = take(icap * 4);
    c.kl_key = take(icap * 4);
    c.dl = take((size_t)3 * PMDI_DL_LDS * 4);
    // ---- sizes that depend on the configuration ----
    c.xs = take((size_t)a.Dmax * 8);
    c.pis = take((size_t)KL * a.N * 8);
    c.term = take((size_t)a.terms_cap * 8);
    c.lw = take((size_t)a.P * 8);
    c.pid = take(a.pid_lds ? (size_t)KL * a.P * 4 : 0);
    c.col = take(a.col_lds ? (size_t)KL * a.P * 4 : 0);
    c.sid = take(a.pp_lds ? (size_t)a.P * 4 : 0);
    c.kv = take(a.pp_lds ? (size_t)a.P * 4 : 0);
    c.lead_of = take((size_t)(a.P + 1) * 4);
    c.slot_of = take((size_t)(a.P + 1) * 4);
    c.cl_lead = take((size_t)KL * PMDI_CLS_LDS * 4);
    c.cl_val = take((size_t)KL * PMDI_CLS_LDS * 4);
    c.bm_fresh = take((size_t)((a.P >> 6) + 1) * 8);
    c.bm_clone = take((size_t)((a.P >> 6) + 1) * 8);
    c.bm_keep = take((size_t)((a.P >> 6) + 1) * 8);
    c.bm_reuse = take((size_t)((a.P >> 6) + 1) * 8);
    c.fl = take((size_t)KL * Dp);
    c.news = take((size_t)KL * a.P);
    c.total = o;
}

}  // namespace

// dynamic LDS of a workgroup of the general kernel with that argument block's layout (the same for every workgroup width)
inline size_t pmdi_sweep_lds_bytes(const SweepArgs &a, int T)
{
    (void)T;
    Carve c;
    carve_lds(a, c);
    return c.total;
}
