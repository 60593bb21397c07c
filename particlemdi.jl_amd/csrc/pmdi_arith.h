// pmdi_arith.h -- the ONE statement of the sweep's pure arithmetic: everything that has to be the same expression, in the same
// order, whichever kernel (or the host) evaluates it, so that a result never depends on which kernel swept a chain:
//   uniform01                                   the counter-based uniforms (Philox4x32-10)
//   gauss_add / gauss_add_sb / gauss_ml /       the Gaussian sufficient-statistic recurrences and the per-feature terms of
//   gauss_term_a / gauss_term_b / gauss_terms   calc_logprob
//   gauss_remove_sb                             the downdate of (Sigma, beta) by the last member added (leave-one-out)
//   negbin_term                                 the NegBinom per-feature term (six look-ups of a loggamma table)
//   resample_u_at                               draw_partstar's u += 1/P sequence, replayed exactly by binade jumps
//   ess_needs_sequential_redo / ess_resamples   the resampling decision
// Plain C++ on scalars (no address spaces, no LDS, no lane operations), usable from the device, the host and the host-side emulation
// of the settled-chain kernel in tests/emu/ (test infrastructure).  Users: pmdi_device.h (namespace pmdi_dev: the general, unit and
// hyper-parameter kernels, through using-declarations and double2 adapters), pmdi_sweep2_body.h (the settled-chain kernel) and
// pmdi_api.cpp (the initial feature flags).  The oracle (oracle/) stays an independent restatement and does not include this file.
// Compile with -ffp-contract=off.  Reference lines are file:line relative to the reference's root.
#pragma once
#include <math.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>      // __umulhi is declared there, not by the compiler
#define PMDI_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define PMDI_HD inline
#endif

namespace pmdi_arith {

// The product of two 32-bit words as its hi and lo words.  On the device MULHI picks how the compiler sees it -- v_mul_hi_u32 and
// v_mul_lo_u32 written out (__umulhi), or one 64-bit product -- the same bits either way, but not the same register allocation around
// it: the general kernel's 128-register build goes from 177 to 193 spill slots with the 64-bit product (tests/test_build_budget.py
// allows 180), and the settled-chain kernel was tuned with it.  Each kernel keeps the form it was measured with: a translation unit
// sets PMDI_ARITH_MULHI (the default of uniform01's MULHI) before it includes this file, or names the form at the call.  The host
// always takes the 64-bit product.
template <bool MULHI>
struct Mul32 {
    unsigned long long m;
    PMDI_HD Mul32(unsigned a, unsigned b) : m((unsigned long long)a * b) {}
    PMDI_HD unsigned hi() const { return (unsigned)(m >> 32); }
    PMDI_HD unsigned lo() const { return (unsigned)m; }
};
#if defined(__HIP_DEVICE_COMPILE__)
template <>
struct Mul32<true> {
    unsigned a, b;
    PMDI_HD Mul32(unsigned a_, unsigned b_) : a(a_), b(b_) {}
    PMDI_HD unsigned hi() const { return __umulhi(a, b); }
    PMDI_HD unsigned lo() const { return a * b; }
};
#endif
#ifndef PMDI_ARITH_MULHI
#define PMDI_ARITH_MULHI false
#endif

// Philox4x32-10, key = (seed lo, seed hi), ctr = (p, pos, site<<16|k, iter): the specification shared with oracle/pmdi_oracle.c.
// MULHI: see Mul32 (pmdi_device.h makes it true for the general, unit and hyper-parameter kernels; the settled-chain kernel asks for false).
template <bool MULHI = PMDI_ARITH_MULHI>
PMDI_HD double uniform01(unsigned long long seed, unsigned iter, unsigned pos, unsigned k, unsigned p, unsigned site)
{
    unsigned c0 = p, c1 = pos, c2 = (site << 16) | k, c3 = iter;
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const Mul32<MULHI> m0(0xD2511F53u, c0), m1(0xCD9E8D57u, c2);
        const unsigned hi0 = m0.hi(), lo0 = m0.lo(), hi1 = m1.hi(), lo1 = m1.lo();
        const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    // 52 random bits -> odd multiple of 2^-53: uniform on the open interval (0,1), never 0
    const unsigned long long m = ((unsigned long long)(c0 >> 6) << 26) | (unsigned long long)(c1 >> 6);
    return (double)(2 * m + 1) * (1.0 / 9007199254740992.0);
}

// cluster_add!(::GaussianCluster), one feature, all four values kept (the stand-alone cluster batches): gaussian_cluster.jl:54-66
PMDI_HD void gauss_add(double x, int nnew, double &mu, double &lam, double &sg, double &bt)
{
    const double n = (double)nnew;
    sg = sg + x;
    const double d = x - mu;
    bt = bt + ((double)(nnew - 1) + 0.001) * (d * d) / (2.0 * (n + 0.001));
    mu = sg / (n + 0.001);
    lam = ((0.5 * n + 0.5) * (n + 0.001)) / (bt * (n + 1.001));
}

// The sweep's pool stores only (Sigma, beta) per feature: mu and lambda are pure functions of (Sigma, beta, n) --
// gaussian_cluster.jl:60-63 recomputes them from exactly these values at every add -- so they are derived on demand, bit-identically,
// and an update touches 16 bytes instead of 64.  (Valid while the feature flags are fixed for the lifetime of the pool, which holds
// inside a sweep: a feature is either updated at every add or never read.)
// cluster_add! on the (Sigma, beta) pair: mu of the previous size is Sigma / (n - 1 + kappa0)
PMDI_HD void gauss_add_sb(double x, int nnew, double &sg, double &bt)
{
    const double n = (double)nnew;
    const double mu_prev = (nnew == 1) ? 0.0 : sg / ((double)(nnew - 1) + 0.001);
    sg = sg + x;
    const double d = x - mu_prev;
    bt = bt + ((double)(nnew - 1) + 0.001) * (d * d) / (2.0 * (n + 0.001));
}

// The algebraic inverse of gauss_add_sb with x as the LAST member added: (Sigma, beta) of a cluster of size cn >= 1 become those of
// the cn - 1 other members (the leave-one-out accumulator's own-label cluster, include/pmdi_hip.h).  beta' repeats the added term
// with the mean of the others, so it agrees with a rebuild from the other members only to rounding -- the subtraction is
// conditioned like beta / beta'  -- and never falls below the constructor's 0.5.  cn == 1: exactly the
// constructor's (0, 0.5), whatever (0.5 + t) - t rounds to.
PMDI_HD void gauss_remove_sb(double x, int cn, double &sg, double &bt)
{
    if (cn == 1) { sg = 0.0; bt = 0.5; return; }
    const double n = (double)cn;
    sg = sg - x;
    const double mu_rest = sg / ((double)(cn - 1) + 0.001);
    const double d = x - mu_rest;
    bt = bt - ((double)(cn - 1) + 0.001) * (d * d) / (2.0 * (n + 0.001));
    bt = (bt > 0.5) ? bt : 0.5;
}

// mu and lambda of a cluster of size cn from (Sigma, beta): gaussian_cluster.jl:60-63 (cn == 0: the constructor's mu = 0, lambda = 1)
PMDI_HD void gauss_ml(int cn, double sg, double bt, double &mu, double &lam)
{
    if (cn == 0) { mu = 0.0; lam = 1.0; return; }
    const double n = (double)cn;
    mu = sg / (n + 0.001);
    lam = ((0.5 * n + 0.5) * (n + 0.001)) / (bt * (n + 1.001));
}

// the two per-feature terms of calc_logprob(::GaussianCluster) for a cluster of size n: gaussian_cluster.jl:45-48.  The first
// depends on the cluster only (the settled-chain kernel caches it per cluster); the second takes d = x - mu (that kernel forms
// the difference before the first term, the general kernel after it: independent operations, but each build keeps the order it had).
PMDI_HD double gauss_term_a(double n, double lam) { return 0.5 * log(lam / (n + 1.0)); }
PMDI_HD double gauss_term_b(double d, double n, double lam) { return (0.5 * n + 1.0) * log(1.0 + (1.0 / (n + 1.0)) * (d * d) * lam); }
PMDI_HD void gauss_terms(double x, double n, double mu, double lam, double &ta, double &tb)
{
    ta = gauss_term_a(n, lam);
    tb = gauss_term_b(x - mu, n, lam);
}

// calc_logprob(::NegBinomCluster) per-feature term: negbinom_cluster.jl:33-37; loggamma of integers comes from the host-built table
// lg[m] = lgamma(m) (Tab: whatever indexes like one -- every caller keeps its typed pointer)
template <class Tab>
PMDI_HD double negbin_term(Tab lg, long long n, long long x, long long S)
{
    return lg[1 + n + 1] + lg[1 + x + S] + lg[1 + n + 1 + S] - lg[1 + n + 1 + 1 + x + S] - lg[1 + n] - lg[1 + S];
}

// draw_partstar's u after j of its `u += 1/particles` (src/misc.jl:34), starting from u01 / P, for P a power of two -- without the
// j additions and still bit-exact: h = 1/P is a power of two, so inside a binade [2^e, 2^(e+1)) every u + h is exact (h is a multiple
// of ulp(u)); only the additions that cross into the next binade round.  Replays the crossings (about ten of them) and jumps over
// the exact runs in between.
PMDI_HD double resample_u_at(double u01, int P, int j)
{
    const double h = 1.0 / (double)P;
    double u = u01 / (double)P;
    int done = 0;
    while (done < j) {
        int e;
        (void)frexp(u, &e);                          // u in [2^(e-1), 2^e)
        const double B = ldexp(1.0, e);
        const double x = (B - u) * (double)P;        // exact: B - u (same binade) and the power-of-two scale
        double m = floor(x);
        if (m == x) m -= 1.0;                        // largest m with u + m*h < B
        if (m > (double)(j - done)) m = (double)(j - done);
        if (m >= 1.0) { u = u + m * h; done += (int)m; }      // exact run inside the binade
        if (done < j) { u = u + h; done += 1; }               // the crossing step rounds like the loop's
    }
    return u;
}

// The resampling decision (src/pmdi.jl:317) on calc_ESS's value (src/misc.jl:15-25).  The kernels' tree-ordered sums agree with
// calc_ESS's sequential loop (src/misc.jl:19-23) to ~1e-13 relative; the decision is a comparison, so when ESS lands that close to
// P/2 -- k equal weights and the rest negligible give exactly k in the reference's order, and k = P/2 does happen -- the sums are
// redone in the reference's order by one lane before ess_resamples is asked.
PMDI_HD bool ess_needs_sequential_redo(double ess, int P) { return fabs(ess - 0.5 * (double)P) <= 1e-9 * (double)P; }
PMDI_HD bool ess_resamples(double ess, int P) { return ess <= 0.5 * (double)P; }

}  // namespace pmdi_arith
