// pmdi_loo.hip -- one add of the streaming leave-one-out accumulator (include/pmdi_hip.h, pmdi_loo_*): how well does the current
// state of every chain explain each TRAINING row, given all the others?  Four kernels per batch of chains:
//   loo_rebuild_kernel     per (chain, dataset, label): the label's cluster rebuilt from its members in ascending observation order
//                          under the chain's feature flags -- the loop of predict_weights_kernel, written a second time (DESIGN.md
//                          4.24) -- with the statistics sent to a global buffer, not evaluated: (Sigma, beta), level counts, sums
//   loo_weights_kernel     the hot path.  A workgroup owns 256 rows of one (chain, dataset), a lane one row.  Features go in tiles of
//                          LW_F in ascending order: the tile of x is staged through LDS (coalesced global read, row stride 17: no
//                          bank conflict), then the occupied labels go in stages of up to LW_LC whose constants -- (mu, lambda, term
//                          a) per feature, or the level counts, or the sums -- are parked in LDS and read as broadcasts by lanes that
//                          walk the same (label, feature).  The empty labels share one value per row, and the row's own label is
//                          evaluated without the row: the lane downdates its label's statistics on the fly (gauss_remove_sb, count
//                          - 1, S - x).  lp gets one store per (row, label) and feature tile, never one per term.
//   loo_normalise_kernel   per (chain, dataset, row): the Gibbs full conditional over the N labels with Pi and, coupled, Phi against
//                          the labels the other datasets give the row; its log normaliser, the fixed-point mass on the own label
//                          and on the labels that are empty once the row is gone
//   loo_accumulate_kernel  one owner lane per (dataset, row), the batch's chains in ascending order: the five sums, the degenerate
//                          rows and the harmonic-mean pair (E, S), exact integer bins.  No atomics.
// The arithmetic is pmdi_arith.h's and the tables are the host-built ones, so a label that is not the row's own has the bits the
// predictive accumulator gives the same row as a new one.  Compile with -ffp-contract=off.
#include "pmdi_device.h"

using namespace pmdi_dev;

namespace {

constexpr int LR_CHUNK = 4096;              // rebuild: observations whose members are listed per pass ...
constexpr int LR_SEG = LR_CHUNK / 4;        // ... a quarter per wave, so the list keeps the observation order
constexpr int LR_TILE_INTS = 10240;         // rebuild: categorical level counts of a tile of features
constexpr int LW_ROWS = 256;                // weights: rows per workgroup, one per lane
constexpr int LW_F = 16;                    // ... features per tile
constexpr int LW_XROW = LW_F + 1;           // ... row stride of the staged tile, in elements: odd, so 8-byte reads of a column spread over all banks
constexpr int LW_LC = 32;                   // ... occupied labels per stage
constexpr int LW_CAT_INTS = 6144;           // ... level counts per stage of a categorical dataset (24 KiB: 58 KiB with the tile of x)

// what calc_logprob starts from for a cluster of size m, before its loop over the features (predict_weights_kernel's expression)
__device__ double loo_start(const DsetDev &d, const unsigned char *fl, int m)
{
    double start = 0.0;
    if (d.kind == K_GAUSSIAN) {
        int nflag = 0;
        for (int q = 0; q < d.D; ++q) nflag += (fl ? fl[q] != 0 : 1);
        start = (double)nflag * glob(d.gtab)[m];
    } else if (d.kind == K_CATEGORICAL) {
        double acc = 0.0;
        for (int q = 0; q < d.D; ++q) {
            if (fl && !fl[q]) continue;
            acc += glob(d.lhtab)[glob(d.maxcol)[q] + 2 * m];
        }
        start = -acc;
    }
    return start;
}

__global__ void __launch_bounds__(256) loo_rebuild_kernel(const LooArgs a, int c0)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int *list = (int *)smem;                                        // [4][LR_SEG] members of the chunk, per wave in ascending order
    int *tile = (int *)(smem + (size_t)LR_CHUNK * 4);               // [ltile][L] level counts of a categorical tile
    __shared__ int s_count, wcount[4];
    const int N = a.N, K = a.K;
    const long long n = a.n;
    const int l = blockIdx.x % N;
    const int k = (blockIdx.x / N) % K;
    const int cb = blockIdx.x / (N * K), c = c0 + cb;
    const DsetDev &d = a.ds[k];
    const int D = d.D, L = d.L, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int *traj = a.s + ((size_t)c * K + k) * n;
    const unsigned char *fl = a.flags ? a.flags + (size_t)c * a.sumD + d.flag_off : nullptr;
    char *st = a.stats + (size_t)cb * a.stat_chain + a.stat_at[k] + (size_t)l * a.stat_label[k];

    // the label's size; any label outside 0..N-1 raises the flag (it is a member of no cluster)
    if (tid == 0) s_count = 0;
    __syncthreads();
    int mine = 0;
    bool bad = false;
    for (long long i = tid; i < n; i += 256) {
        const int v = traj[i];
        mine += (v == l);
        bad |= ((unsigned)v >= (unsigned)N);
    }
    if (mine) atomicAdd(&s_count, mine);
    if (bad) *a.err = 1;
    __syncthreads();
    const int cn = s_count;
    if (tid == 0) a.cn[((size_t)c * K + k) * N + l] = cn;
    if (tid < 3) {                                                  // at the label's size, with one member less, and empty
        const int m = tid == 0 ? cn : tid == 1 ? (cn > 0 ? cn - 1 : 0) : 0;
        a.start[((((size_t)cb * K + k) * N + l) << 2) + tid] = loo_start(d, fl, m);
    }

    const int Dt = d.kind == K_CATEGORICAL ? a.ltile : 256;
    const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    for (int q0 = 0; q0 < D; q0 += Dt) {
        const int dq = min(Dt, D - q0);
        const int q = q0 + tid;                                     // this lane's feature (Gaussian, NegBinom)
        const bool on = tid < dq && (fl ? fl[q] != 0 : true);
        double sg = 0.0, bt = 0.5;
        long long S = 0;
        int cm = 0;                                                 // members added so far
        if (d.kind == K_CATEGORICAL)
            for (int e = tid; e < dq * L; e += 256) tile[e] = 0;
        __syncthreads();
        if (cn > 0)
            for (long long base = 0; base < n; base += LR_CHUNK) {
                int wc = 0;
                const long long seg = base + (long long)wave * LR_SEG;
                for (int sp = 0; sp < LR_SEG; sp += 64) {
                    const long long i = seg + sp + lane;
                    const bool f = i < n && traj[i] == l;
                    const unsigned long long b = __ballot(f);
                    if (f) list[wave * LR_SEG + wc + __popcll(b & below)] = (int)i;
                    wc += __popcll(b);
                }
                if (lane == 0) wcount[wave] = wc;
                __syncthreads();
                for (int w = 0; w < 4; ++w) {
                    const int nw = wcount[w];
                    const int *mem = list + w * LR_SEG;
                    if (d.kind == K_GAUSSIAN) {
                        if (on) {                                   // four members' values in flight, added in order
                            int t = 0;
                            for (; t + 4 <= nw; t += 4) {
                                const double x0 = glob(d.xf)[(size_t)mem[t] * D + q], x1 = glob(d.xf)[(size_t)mem[t + 1] * D + q];
                                const double x2 = glob(d.xf)[(size_t)mem[t + 2] * D + q], x3 = glob(d.xf)[(size_t)mem[t + 3] * D + q];
                                pmdi_arith::gauss_add_sb(x0, cm + 1, sg, bt);
                                pmdi_arith::gauss_add_sb(x1, cm + 2, sg, bt);
                                pmdi_arith::gauss_add_sb(x2, cm + 3, sg, bt);
                                pmdi_arith::gauss_add_sb(x3, cm + 4, sg, bt);
                                cm += 4;
                            }
                            for (; t < nw; ++t) {
                                ++cm;
                                pmdi_arith::gauss_add_sb(glob(d.xf)[(size_t)mem[t] * D + q], cm, sg, bt);
                            }
                        }
                    } else if (d.kind == K_NEGBINOM) {
                        if (on)
                            for (int t = 0; t < nw; ++t) S += glob(d.xi)[(size_t)mem[t] * D + q];
                    } else {                                        // integer counts: exact in any order, every lane helps
                        for (int e = tid; e < nw * dq; e += 256) {
                            const int t = e / dq, qq = e - t * dq;
                            if (fl && !fl[q0 + qq]) continue;
                            atomicAdd(&tile[qq * L + (glob(d.xi)[(size_t)mem[t] * D + q0 + qq] - 1)], 1);
                        }
                    }
                }
                __syncthreads();
            }
        if (d.kind == K_GAUSSIAN) {
            if (tid < dq) { ((double *)st)[2 * (size_t)q] = sg; ((double *)st)[2 * (size_t)q + 1] = bt; }
        } else if (d.kind == K_NEGBINOM) {
            if (tid < dq) ((long long *)st)[q] = S;
        } else {
            for (int e = tid; e < dq * L; e += 256) ((int *)st)[(size_t)q0 * L + e] = tile[e];
        }
        __syncthreads();
    }
}

// The per-feature term of calc_logprob for one row value against a cluster given by its statistics: the expressions of
// predict_weights_kernel.  Gaussian: (mu, lambda) and term a = gauss_term_a(n, lambda); Categorical: the count of the row's level;
// NegBinom: the sum.
template <int KIND>
struct LooVal { typedef int type; };
template <>
struct LooVal<K_GAUSSIAN> { typedef double type; };

template <int KIND>
__device__ void loo_weights_body(const LooArgs &a, const DsetDev &d, int c0, unsigned char *smem)
{
    typedef typename LooVal<KIND>::type X;
    __shared__ int occ[256];                                        // the occupied labels, ascending (N <= 255)
    __shared__ int s_nocc, lab_l[LW_LC], lab_n[LW_LC];
    __shared__ double lab_start[LW_LC];
    const int N = a.N, K = a.K, tid = threadIdx.x;
    const long long n = a.n;
    const int k = blockIdx.y, cb = blockIdx.z, c = c0 + cb;
    const long long i0 = (long long)blockIdx.x * LW_ROWS, i = i0 + tid;
    const bool valid = i < n;
    const int D = d.D, L = d.L;
    const unsigned char *fl = a.flags ? a.flags + (size_t)c * a.sumD + d.flag_off : nullptr;
    const int *traj = a.s + ((size_t)c * K + k) * n;
    const int *cnv = a.cn + ((size_t)c * K + k) * N;
    const double *stv = a.start + (((size_t)cb * K + k) * N << 2);
    const char *st = a.stats + (size_t)cb * a.stat_chain + a.stat_at[k];
    const size_t sl = a.stat_label[k];
    double *lp = a.lp + ((((size_t)(a.lp_all ? c : cb) * K + k) * n) + (valid ? i : 0)) * N;      // this lane's row
    X *xs = (X *)smem;                                              // [LW_ROWS][LW_XROW]
    unsigned char *cst = smem + (size_t)LW_ROWS * LW_XROW * 8;      // the stage's constants
    const X *xg = KIND == K_GAUSSIAN ? (const X *)d.xf : (const X *)d.xi;

    if (tid == 0) {
        int m = 0;
        for (int l = 0; l < N; ++l)
            if (cnv[l] > 0) occ[m++] = l;
        s_nocc = m;
    }
    int o = valid ? traj[i] : -1;                                   // the row's own label; a label outside 0..N-1 is no cluster's
    if ((unsigned)o >= (unsigned)N) o = -1;
    const int cno = o >= 0 ? cnv[o] : 0;
    const char *sto = st + (size_t)(o >= 0 ? o : 0) * sl;
    double out_own = 0.0, out_e = 0.0;
    __syncthreads();
    const int nocc = s_nocc;

    const int Dt = KIND == K_CATEGORICAL ? min(LW_F, LW_CAT_INTS / L) : LW_F;       // L <= 4096: at least one feature
    const int lstage = KIND == K_CATEGORICAL ? max(1, min(LW_LC, LW_CAT_INTS / (min(Dt, D) * L))) : LW_LC;
    for (int q0 = 0; q0 < D; q0 += Dt) {
        const int dq = min(Dt, D - q0);
        unsigned onmask = 0;
        for (int qq = 0; qq < dq; ++qq) onmask |= (unsigned)(fl ? fl[q0 + qq] != 0 : 1) << qq;
        __syncthreads();                                            // the last tile's readers are done
        for (int e = tid; e < LW_ROWS * dq; e += 256) {
            const int r = e / dq, qq = e - r * dq;
            const long long row = i0 + r;
            xs[r * LW_XROW + qq] = row < n ? glob(xg)[(size_t)row * D + q0 + qq] : (X)0;
        }
        __syncthreads();
        const X *xr = xs + tid * LW_XROW;
        if (q0 == 0) {
            out_e = stv[2];
            out_own = o >= 0 ? stv[((size_t)o << 2) + 1] : 0.0;
        }
        if (valid) {
            // the row's own label without the row, and the empty cluster: no shared constants, the lane forms them
            for (int qq = 0; qq < dq; ++qq) {
                if (!((onmask >> qq) & 1u)) continue;
                const int f = q0 + qq;
                if constexpr (KIND == K_GAUSSIAN) {
                    const double x = xr[qq];
                    double ta, tb;
                    if (o >= 0) {
                        double sg = glob((const double *)sto)[2 * (size_t)f], bt = glob((const double *)sto)[2 * (size_t)f + 1], mu, lam;
                        pmdi_arith::gauss_remove_sb(x, cno, sg, bt);
                        pmdi_arith::gauss_ml(cno - 1, sg, bt, mu, lam);
                        pmdi_arith::gauss_terms(x, (double)(cno - 1), mu, lam, ta, tb);
                        out_own += ta; out_own -= tb;
                    }
                    pmdi_arith::gauss_terms(x, 0.0, 0.0, 1.0, ta, tb);
                    out_e += ta; out_e -= tb;
                } else if constexpr (KIND == K_CATEGORICAL) {
                    const int x = xr[qq];
                    if (o >= 0) {
                        const int cnt = glob((const int *)sto)[(size_t)f * L + (x - 1)] - 1;
                        out_own += (cno - 1 == 0) ? glob(d.lhtab)[1] : glob(d.lhtab)[2 * cnt + 1];
                    }
                    out_e += glob(d.lhtab)[1];
                } else {
                    const int x = xr[qq];
                    if (o >= 0) out_own += negbin_term(glob(d.lgtab), cno - 1, x, glob((const long long *)sto)[f] - x);
                    out_e += negbin_term(glob(d.lgtab), 0, x, 0);
                }
            }
        }
        // the occupied labels, a stage at a time
        for (int l0 = 0; l0 < nocc; l0 += lstage) {
            const int lc = min(lstage, nocc - l0);
            __syncthreads();                                        // the last stage's readers are done
            if (tid < lc) {
                const int l = occ[l0 + tid];
                lab_l[tid] = l; lab_n[tid] = cnv[l]; lab_start[tid] = stv[(size_t)l << 2];
            }
            if constexpr (KIND == K_GAUSSIAN) {
                for (int e = tid; e < lc * dq; e += 256) {
                    const int ll = e / dq, qq = e - ll * dq, l = occ[l0 + ll];
                    const double *sb = (const double *)(st + (size_t)l * sl) + 2 * (size_t)(q0 + qq);
                    double mu, lam;
                    pmdi_arith::gauss_ml(cnv[l], glob(sb)[0], glob(sb)[1], mu, lam);
                    double *dst = (double *)cst + (ll * LW_F + qq) * 3;
                    dst[0] = mu; dst[1] = lam; dst[2] = pmdi_arith::gauss_term_a((double)cnv[l], lam);
                }
            } else if constexpr (KIND == K_NEGBINOM) {
                for (int e = tid; e < lc * dq; e += 256) {
                    const int ll = e / dq, qq = e - ll * dq, l = occ[l0 + ll];
                    ((long long *)cst)[ll * LW_F + qq] = glob((const long long *)(st + (size_t)l * sl))[q0 + qq];
                }
            } else {
                const int per = dq * L;                             // the tile's counts of one label are contiguous
                for (int e = tid; e < lc * per; e += 256) {
                    const int ll = e / per, r = e - ll * per, l = occ[l0 + ll];
                    ((int *)cst)[e] = glob((const int *)(st + (size_t)l * sl))[(size_t)q0 * L + r];
                }
            }
            __syncthreads();
            if (valid)
                for (int ll = 0; ll < lc; ++ll) {
                    const int l = lab_l[ll], cnl = lab_n[ll];
                    double out = q0 == 0 ? lab_start[ll] : lp[l];
                    if (l == o) out = out_own;                      // (its own terms were summed above)
                    else
                        for (int qq = 0; qq < dq; ++qq) {
                            if (!((onmask >> qq) & 1u)) continue;
                            if constexpr (KIND == K_GAUSSIAN) {
                                const double *cs = (const double *)cst + (ll * LW_F + qq) * 3;
                                out += cs[2]; out -= pmdi_arith::gauss_term_b(xr[qq] - cs[0], (double)cnl, cs[1]);
                            } else if constexpr (KIND == K_CATEGORICAL) {
                                out += glob(d.lhtab)[2 * ((const int *)cst)[(ll * dq + qq) * L + (xr[qq] - 1)] + 1];
                            } else {
                                out += negbin_term(glob(d.lgtab), cnl, xr[qq], ((const long long *)cst)[ll * LW_F + qq]);
                            }
                        }
                    lp[l] = out;
                }
        }
    }
    if (valid)                                                      // every empty label: the constructor's cluster, formed once
        for (int l = 0; l < N; ++l)
            if (cnv[l] == 0) lp[l] = out_e;
}

__global__ void __launch_bounds__(256) loo_weights_kernel(const LooArgs a, int c0)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const DsetDev &d = a.ds[blockIdx.y];
    if (d.kind == K_GAUSSIAN) loo_weights_body<K_GAUSSIAN>(a, d, c0, smem);
    else if (d.kind == K_CATEGORICAL) loo_weights_body<K_CATEGORICAL>(a, d, c0, smem);
    else loo_weights_body<K_NEGBINOM>(a, d, c0, smem);
}

// l -> (e, mant): -l in units of log 2, split into its floor and 2^fraction
__device__ __forceinline__ void loo_split(double ell, long long &e, double &mant)
{
    const double t = (-ell) * 1.4426950408889634;
    double ef = floor(t);
    ef = ef > 1.0e15 ? 1.0e15 : ef < -1.0e15 ? -1.0e15 : ef;       // (no log density gets there; the conversion below stays defined)
    e = (long long)ef;
    mant = exp2(t - ef);
}

// The exact sum of mant 2^e.  mant is an integer m of at most 54 bits times 2^-52; the term m 2^(e - 52) goes to the bin of its
// exponent, bin = floor(e / 32), as the 128-bit integer m << (e mod 32).  A pair keeps the LOO_BINS highest bins seen (E = the
// highest bin index; S[2 j], S[2 j + 1] = the high and low words of bin E - j).  Integer sums per absolute bin are exact, and a
// bin that falls out of the window is dropped whole and never comes back (E only grows): the state is a function of the
// multiset of terms, whatever the order, the batching, or the merges.
constexpr int LOO_BINS = 3;
struct LooBins {                                                    // (named words, not an array: they stay in registers)
    unsigned long long h0, l0, h1, l1, h2, l2;
    __device__ __forceinline__ void load(const long long *p) { h0 = p[0]; l0 = p[1]; h1 = p[2]; l1 = p[3]; h2 = p[4]; l2 = p[5]; }
    __device__ __forceinline__ void store(long long *p) const { p[0] = h0; p[1] = l0; p[2] = h1; p[3] = l1; p[4] = h2; p[5] = l2; }
};
__device__ __forceinline__ void loo_add128(unsigned long long &h, unsigned long long &l, unsigned long long hi, unsigned long long lo)
{
    l = l + lo;
    h = h + hi + (l < lo ? 1ull : 0ull);
}
__device__ __forceinline__ void loo_bin_add(long long &E, LooBins &S, long long bin, unsigned long long hi, unsigned long long lo)
{
    if (E == PMDI_LOO_E_EMPTY_I || bin > E) {                       // the window moves up by d bins
        const long long d = E == PMDI_LOO_E_EMPTY_I ? LOO_BINS : bin - E;
        if (d == 1) { S.h2 = S.h1; S.l2 = S.l1; S.h1 = S.h0; S.l1 = S.l0; }
        else if (d == 2) { S.h2 = S.h0; S.l2 = S.l0; S.h1 = 0; S.l1 = 0; }
        else { S.h2 = 0; S.l2 = 0; S.h1 = 0; S.l1 = 0; }
        S.h0 = 0; S.l0 = 0;
        E = bin;
    }
    const long long d = E - bin;
    if (d == 0) loo_add128(S.h0, S.l0, hi, lo);
    else if (d == 1) loo_add128(S.h1, S.l1, hi, lo);
    else if (d == 2) loo_add128(S.h2, S.l2, hi, lo);
}

__device__ __forceinline__ void loo_pair_add(long long &E, LooBins &S, long long e, double mant)
{
    const unsigned long long m = (mant >= 0.0 && mant < 4.0) ? (unsigned long long)(mant * 4503599627370496.0) : 0ull;
    const int r = (int)(e & 31);
    loo_bin_add(E, S, e >> 5, r ? m >> (64 - r) : 0ull, m << r);
}

// One lane per (chain of the batch, dataset, row)
__global__ void __launch_bounds__(256) loo_normalise_kernel(const LooArgs a, int c0, int chains)
{
    const int N = a.N, K = a.K;
    const long long n = a.n;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)chains * K * n) return;
    const long long i = idx % n;
    const int k = (int)((idx / n) % K), cb = (int)(idx / (n * K)), c = c0 + cb;
    const size_t row = ((size_t)(a.lp_all ? c : cb) * K + k) * n + i;
    const double *lp = a.lp + row * N;
    const double *Pi = a.Pi + ((size_t)c * K + k) * N;
    const int *cn = a.cn + ((size_t)c * K + k) * N;
    const int *sc = a.s + (size_t)c * K * n + i;                    // the row's label in dataset b: sc[b n]
    const bool coupled = a.Phi != nullptr && K > 1;
    const double *Phi = coupled ? a.Phi + (size_t)c * a.npairs : nullptr;
    int o = sc[(size_t)k * n];
    if ((unsigned)o >= (unsigned)N) o = -1;
    // the row's labels in the other datasets and their Phi, in registers (constant bounds: the loops unroll, nothing is indexed)
    int sb[PMDI_KMAX_I];
    double ph[PMDI_KMAX_I];
#pragma unroll
    for (int b = 0; b < PMDI_KMAX_I; ++b) {
        sb[b] = -1; ph[b] = 0.0;
        if (coupled && b < K && b != k) {
            const int lo = b < k ? b : k, hi = b < k ? k : b;
            sb[b] = sc[(size_t)b * n];
            ph[b] = Phi[lo * K - lo * (lo + 1) / 2 + (hi - lo - 1)];
        }
    }
    auto weight_u = [&](int l) {
        double u = 1.0;
        if (coupled) {
#pragma unroll
            for (int b = 0; b < PMDI_KMAX_I; ++b)
                if (b < K && b != k) u = u * (1.0 + ph[b] * (sb[b] == l ? 1.0 : 0.0));
        }
        return u;
    };
    double mx = lp[0];
    for (int l = 1; l < N; ++l) { const double v = lp[l]; mx = (v > mx) ? v : mx; }
    double F = 0.0, Z0 = 0.0;
    for (int l = 0; l < N; ++l) {
        const double u = weight_u(l);
        const double w = exp(lp[l] - mx) * Pi[l] * u, z = Pi[l] * u;
        F = l == 0 ? w : F + w;
        Z0 = l == 0 ? z : Z0 + z;
    }
    double ell = log(F) + mx;
    if (coupled) ell -= log(Z0);
    int pown = 0, pnew = 0;
    if (F > 0.0 && F <= 1.7976931348623157e308) {
        for (int l = 0; l < N; ++l) {
            const bool own = l == o, gone = cn[l] == 0 || (own && cn[l] == 1);
            if (!own && !gone) continue;
            const double w = exp(lp[l] - mx) * Pi[l] * weight_u(l);
            const int qv = (int)floor(w / F * 1048576.0 + 0.5);
            if (own) pown = qv;
            if (gone) pnew += qv;
        }
    } else {
        pown = -1;                                                  // a degenerate row: it counts in `zero` and nowhere else
    }
    a.ell[row] = ell;
    a.pown[row] = pown;
    a.pnew[row] = pnew;
    if (a.e_last) {
        long long e;
        double mant;
        loo_split(ell, e, mant);
        a.e_last[row] = e;
        a.mant_last[row] = mant;
    }
}

// One lane per (dataset, row): the batch's chains in ascending order
__global__ void __launch_bounds__(256) loo_accumulate_kernel(const LooArgs a, int c0, int chains)
{
    const long long Kn = (long long)a.K * a.n;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= Kn) return;
    long long own = a.own_sum[idx], nw = a.new_sum[idx], zero = a.zero[idx], E = a.E[idx];
    double lcp = a.lcp_sum[idx], lsq = a.lcp_sq_sum[idx];
    LooBins S;
    S.load(a.S + idx * (2 * LOO_BINS));
    for (int cb = 0; cb < chains; ++cb) {
        const size_t row = (size_t)(a.lp_all ? c0 + cb : cb) * Kn + idx;
        const int po = a.pown[row];
        if (po < 0) { zero += 1; continue; }
        const double ell = a.ell[row];
        own += po;
        nw += a.pnew[row];
        lcp = lcp + ell;
        lsq = lsq + ell * ell;
        long long e;
        double mant;
        loo_split(ell, e, mant);
        loo_pair_add(E, S, e, mant);
    }
    a.own_sum[idx] = own; a.new_sum[idx] = nw; a.zero[idx] = zero; a.E[idx] = E;
    a.lcp_sum[idx] = lcp; a.lcp_sq_sum[idx] = lsq;
    S.store(a.S + idx * (2 * LOO_BINS));
}

__global__ void __launch_bounds__(256) loo_merge_kernel(const LooArgs a, const long long *__restrict__ own_b, const long long *__restrict__ new_b,
                                                        const long long *__restrict__ zero_b, const double *__restrict__ lcp_b,
                                                        const double *__restrict__ lcpsq_b, const long long *__restrict__ E_b,
                                                        const long long *__restrict__ S_b)
{
    const long long Kn = (long long)a.K * a.n;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= Kn) return;
    a.own_sum[idx] += own_b[idx];
    a.new_sum[idx] += new_b[idx];
    a.zero[idx] += zero_b[idx];
    a.lcp_sum[idx] = a.lcp_sum[idx] + lcp_b[idx];
    a.lcp_sq_sum[idx] = a.lcp_sq_sum[idx] + lcpsq_b[idx];
    if (E_b[idx] != PMDI_LOO_E_EMPTY_I) {
        long long E = a.E[idx];
        LooBins S;
        S.load(a.S + idx * (2 * LOO_BINS));
#pragma unroll
        for (int j = 0; j < LOO_BINS; ++j)                           // their bins, highest first, each as one term of its bin
            loo_bin_add(E, S, E_b[idx] - j, (unsigned long long)S_b[idx * (2 * LOO_BINS) + 2 * j], (unsigned long long)S_b[idx * (2 * LOO_BINS) + 2 * j + 1]);
        a.E[idx] = E;
        S.store(a.S + idx * (2 * LOO_BINS));
    }
}

}  // namespace

hipError_t pmdi_launch_loo_add(const LooArgs &a, hipStream_t stream)
{
    LooArgs b = a;
    int Lmax = 1;
    bool cat = false;
    for (int k = 0; k < a.K; ++k)
        if (a.ds[k].kind == K_CATEGORICAL) { cat = true; if (a.ds[k].L > Lmax) Lmax = a.ds[k].L; }
    b.ltile = LR_TILE_INTS / Lmax;                                  // L <= 4096 (pmdi_create): at least two features per tile
    if (b.ltile > 256) b.ltile = 256;
    size_t tile_bytes = 16;
    for (int k = 0; k < a.K; ++k)
        if (a.ds[k].kind == K_CATEGORICAL) {
            const size_t need = (size_t)(a.ds[k].D < b.ltile ? a.ds[k].D : b.ltile) * a.ds[k].L * 4;
            if (need > tile_bytes) tile_bytes = need;
        }
    const size_t lds_r = (size_t)LR_CHUNK * 4 + ((tile_bytes + 15) & ~(size_t)15);
    // the staged tile of x (as doubles: the widest kind) and one stage's constants
    const size_t lds_w = (size_t)LW_ROWS * LW_XROW * 8 + (cat ? (size_t)LW_CAT_INTS * 4 : (size_t)LW_LC * LW_F * 24);
    const long long Kn = (long long)a.K * a.n;
    for (int c0 = 0; c0 < a.C; c0 += a.Cb) {
        const int chains = a.C - c0 < a.Cb ? a.C - c0 : a.Cb;
        hipLaunchKernelGGL(loo_rebuild_kernel, dim3((unsigned)chains * a.K * a.N), dim3(256), lds_r, stream, b, c0);
        hipLaunchKernelGGL(loo_weights_kernel, dim3((unsigned)((a.n + LW_ROWS - 1) / LW_ROWS), (unsigned)a.K, (unsigned)chains), dim3(256),
                           lds_w, stream, b, c0);
        hipLaunchKernelGGL(loo_normalise_kernel, dim3((unsigned)((chains * Kn + 255) / 256)), dim3(256), 0, stream, b, c0, chains);
        hipLaunchKernelGGL(loo_accumulate_kernel, dim3((unsigned)((Kn + 255) / 256)), dim3(256), 0, stream, b, c0, chains);
    }
    return hipGetLastError();
}

hipError_t pmdi_launch_loo_merge(const LooArgs &a, const long long *own_b, const long long *new_b, const long long *zero_b,
                                 const double *lcp_b, const double *lcpsq_b, const long long *E_b, const long long *S_b, hipStream_t stream)
{
    const long long Kn = (long long)a.K * a.n;
    hipLaunchKernelGGL(loo_merge_kernel, dim3((unsigned)((Kn + 255) / 256)), dim3(256), 0, stream, a, own_b, new_b, zero_b, lcp_b, lcpsq_b,
                       E_b, S_b);
    return hipGetLastError();
}
