// pmdi_density.hip -- one add of the streaming density accumulator (include/pmdi_hip.h, pmdi_density_*): the log density of the
// state every chain is in.  Per add:
//   density_stats_kernel    the hot path, one workgroup per (chain, dataset).  A histogram pass gives cn[l] and first[l]; then the
//                           features go in tiles.  Per tile the rows go in chunks of DS_CHUNK: a chunk is partitioned stably by
//                           label into member lists in LDS (ballots and popcounts, the waves in row order), and the (label,
//                           feature) items of the tile are dealt to the lanes, adjacent lanes adjacent features: a lane walks its
//                           own label's list and carries the running (Sigma, beta) -- or the NegBinom sum -- of its item in LDS from
//                           chunk to chunk.  The labels are read once per feature tile, not once per label as featsel_label_kernel
//                           (pmdi_kernels.hip) reads them.  Categorical level counts are integers, exact in any order: every
//                           lane adds rows of the chunk into an LDS tile of (label, feature, level) counts, tiled over features and
//                           levels.  Each item ends in calc_logmarginal of its cluster, lm[l][q] -- the expressions of
//                           pmdi_kernels.hip's logmarginal_one, written a second time (that file is untouched).
//   density_feature_kernel  one lane per (chain, feature): bf and cl over the labels by ascending first[l], and q
//   density_agree_kernel    one wavefront per (chain, pair): rows the two datasets label alike
//   density_chain_kernel    one working lane per chain: ll[k], Z by the subset recursions of pmdi_subset.h, lprior, lj, the trace
//                           rows and the decision whether this state is the chain's best
//   density_best_kernel     the conditional copy of the allocations
//   density_sums_kernel     one owner lane per feature, the chains in ascending order.  No atomics on doubles anywhere.
// The chains go through the first two kernels in batches (the stage buffer lm); every other kernel is sequential in the chains or
// independent per chain, so no result depends on the batching or on a launch shape.  Compile with -ffp-contract=off.
#include "pmdi_device.h"
#include "pmdi_subset.h"

using namespace pmdi_dev;

namespace {

constexpr int DS_CHUNK = 2048;              // rows partitioned per pass ...
constexpr int DS_SEG = DS_CHUNK / 4;        // ... a quarter per wave, so the lists keep the row order
constexpr int DS_FT = 64;                   // features per tile, at most
constexpr int DS_ITEMS = 2048;              // (label, feature) items whose running statistics a tile holds: 16 bytes each
constexpr int DS_CAT_INTS = 8192;           // level counts of one (feature, level) tile of a categorical dataset
constexpr size_t DS_LDS = (size_t)DS_ITEMS * 8 + (size_t)DS_CAT_INTS * 4;     // 48 KiB: [items] doubles + the counts, or [items] pairs

// features per tile when `nocc` labels are occupied (>= 1), and for a categorical dataset the levels per tile
__device__ __forceinline__ void ds_tile(int kind, int nocc, int L, int &ft, int &lt)
{
    ft = min(DS_FT, max(1, DS_ITEMS / nocc));                       // nocc <= 255: at least 8
    lt = 1;
    if (kind == K_CATEGORICAL) {
        lt = min(L, max(1, DS_CAT_INTS / nocc));                    // at least 32
        ft = min(ft, max(1, DS_CAT_INTS / (nocc * lt)));
    }
}

__global__ void __launch_bounds__(256) density_stats_kernel(const DensityArgs a, int c0)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ unsigned short list[DS_CHUNK];                       // the chunk's rows (chunk-local), label by label, ascending in each
    __shared__ int wcnt[4 * 256];                                   // [wave][label]: the wave's members, then its cursor into list
    __shared__ int s_cn[256], s_first[256], lab_off[256], lab_cnt[256], before[256], occ[256], occ_of[256];
    __shared__ unsigned long long scr[4];
    __shared__ int s_nocc;
    const int N = a.N, K = a.K, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long n = a.n;
    const int k = blockIdx.x % K, cb = blockIdx.x / K, c = c0 + cb;
    const DsetDev &d = a.ds[k];
    const int D = d.D, L = d.L, kind = d.kind;
    const int *traj = a.s + ((size_t)c * K + k) * n;
    double *lm = a.lm + ((size_t)(a.lm_all ? c : cb) * a.sumD + d.flag_off) * N;    // [q][l] of this dataset
    double *runs = (double *)smem;                                  // Gaussian [item] (Sigma, beta); NegBinom [item] sum; Categorical [item] value
    int *lev = (int *)(smem + (size_t)DS_ITEMS * 8);                // Categorical [label][feature][level] counts of the tile

    // cn and first of every label; a label outside 0..N-1 raises the flag (it is a member of no cluster)
    s_cn[tid] = 0; s_first[tid] = PMDI_INF_I;
    __syncthreads();
    bool bad = false;
    for (long long i = tid; i < n; i += 256) {
        const int v = traj[i];
        if ((unsigned)v < (unsigned)N) { atomicAdd(&s_cn[v], 1); atomicMin(&s_first[v], (int)i); }
        else bad = true;
    }
    if (bad) *a.err = 1;
    __syncthreads();
    if (tid == 0) {
        int m = 0;
        for (int l = 0; l < N; ++l)
            if (s_cn[l] > 0) { occ_of[l] = m; occ[m++] = l; }
        s_nocc = m;
    }
    __syncthreads();
    const int nocc = s_nocc;
    if (tid < N) {
        const size_t at = ((size_t)c * K + k) * N;
        a.cn[at + tid] = s_cn[tid];
        a.first[at + tid] = s_first[tid];
        if (s_cn[tid] > 0) {                                        // the occupied labels by first appearance: the firsts are distinct
            int r = 0;
            for (int l = 0; l < N; ++l) r += (s_first[l] < s_first[tid]);
            a.ord[at + r] = tid;
        }
        if (tid == 0) a.nocc[(size_t)c * K + k] = nocc;
    }
    for (int e = tid; e < N * D; e += 256) {                        // an empty label has no cluster: 0.0, which adds nothing
        const int l = e % N, q = e / N;
        if (s_cn[l] == 0) lm[(size_t)q * N + l] = 0.0;
    }
    if (nocc == 0) return;

    int Ft, Lt;
    ds_tile(kind, nocc, L, Ft, Lt);
    const int nlt = kind == K_CATEGORICAL ? (L + Lt - 1) / Lt : 1;
    const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    volatile int *cur = wcnt + wave * 256;
    for (int q0 = 0; q0 < D; q0 += Ft) {
        const int dq = min(Ft, D - q0), items = nocc * dq;
        for (int e = tid; e < items; e += 256) {
            if (kind == K_GAUSSIAN) { runs[2 * e] = 0.0; runs[2 * e + 1] = 0.5; }
            else if (kind == K_NEGBINOM) ((long long *)runs)[e] = 0;
            else {
                const int o = e / dq, qq = e - o * dq;
                const int mc = glob(d.maxcol)[q0 + qq];
                double val = 0.0;
                val += glob(d.lghtab)[2 * mc] - glob(d.lghtab)[2 * (mc + s_cn[occ[o]])];
                runs[e] = val;
            }
        }
        for (int lt = 0; lt < nlt; ++lt) {
            const int l0 = lt * Lt;
            if (kind == K_CATEGORICAL)
                for (int e = tid; e < items * Lt; e += 256) lev[e] = 0;
            before[tid] = 0;
            __syncthreads();
            for (long long base = 0; base < n; base += DS_CHUNK) {
                const int rows = (int)min((long long)DS_CHUNK, n - base);
                if (kind == K_CATEGORICAL) {                        // integer counts: exact in any order, every lane helps
                    for (int e = tid; e < rows * dq; e += 256) {
                        const int r = e / dq, qq = e - r * dq;
                        const int v = traj[base + r];
                        if ((unsigned)v >= (unsigned)N) continue;
                        const int x = glob(d.xi)[(size_t)(base + r) * D + q0 + qq] - 1 - l0;
                        if (x >= 0 && x < Lt) atomicAdd(&lev[(occ_of[v] * dq + qq) * Lt + x], 1);
                    }
                    continue;
                }
                // the chunk's rows, partitioned stably by label: count per (wave, label) ...
                for (int e = tid; e < 4 * 256; e += 256) wcnt[e] = 0;
                __syncthreads();
                for (int sp = 0; sp < DS_SEG; sp += 64) {
                    const int r = wave * DS_SEG + sp + lane;
                    const int v = r < rows ? traj[base + r] : -1;
                    if ((unsigned)v < (unsigned)N) atomicAdd(&wcnt[wave * 256 + v], 1);
                }
                __syncthreads();
                // ... the labels' offsets into the list, and every wave's cursor ...
                const int tot = tid < N ? wcnt[tid] + wcnt[256 + tid] + wcnt[512 + tid] + wcnt[768 + tid] : 0;
                unsigned long long total;
                const int off = (int)block_excl_scan<256>((unsigned long long)tot, total, scr);
                if (tid < N) {
                    lab_off[tid] = off; lab_cnt[tid] = tot;
                    int at = off;
                    for (int w = 0; w < 4; ++w) { const int t = wcnt[w * 256 + tid]; wcnt[w * 256 + tid] = at; at += t; }
                }
                __syncthreads();
                // ... and every row to its place: lanes of one label take consecutive slots in lane order
                for (int sp = 0; sp < DS_SEG; sp += 64) {
                    const int r = wave * DS_SEG + sp + lane;
                    const int v = r < rows ? traj[base + r] : -1;
                    const bool valid = (unsigned)v < (unsigned)N;
                    unsigned long long active = __ballot(valid);
                    int rank = 0, mine_n = 0;
                    bool leader = false;
                    while (active) {
                        const int f0 = __ffsll((long long)active) - 1;
                        const int v0 = __builtin_amdgcn_readlane(v, f0);
                        const bool mine = valid && v == v0;
                        const unsigned long long m = __ballot(mine);
                        if (mine) rank = __popcll(m & below);
                        if (lane == f0) { leader = true; mine_n = __popcll(m); }
                        active &= ~m;
                    }
                    if (valid) list[cur[v] + rank] = (unsigned short)r;
                    if (leader) cur[v] = cur[v] + mine_n;           // (one wave's LDS accesses complete in order)
                }
                __syncthreads();
                // the items: a lane adds the members of its label to its feature, in row order
                for (int e = tid; e < items; e += 256) {
                    const int o = e / dq, qq = e - o * dq, l = occ[o];
                    const int nw = lab_cnt[l];
                    if (nw == 0) continue;
                    const unsigned short *mem = list + lab_off[l];
                    const size_t col = (size_t)base * D + q0 + qq;
                    if (kind == K_GAUSSIAN) {
                        const double *x = d.xf + col;
                        double sg = runs[2 * e], bt = runs[2 * e + 1];
                        int cm = before[l], t = 0;
                        for (; t + 4 <= nw; t += 4) {               // four members' values in flight, added in order
                            const double x0 = glob(x)[(size_t)mem[t] * D], x1 = glob(x)[(size_t)mem[t + 1] * D];
                            const double x2 = glob(x)[(size_t)mem[t + 2] * D], x3 = glob(x)[(size_t)mem[t + 3] * D];
                            pmdi_arith::gauss_add_sb(x0, cm + 1, sg, bt);
                            pmdi_arith::gauss_add_sb(x1, cm + 2, sg, bt);
                            pmdi_arith::gauss_add_sb(x2, cm + 3, sg, bt);
                            pmdi_arith::gauss_add_sb(x3, cm + 4, sg, bt);
                            cm += 4;
                        }
                        for (; t < nw; ++t) {
                            ++cm;
                            pmdi_arith::gauss_add_sb(glob(x)[(size_t)mem[t] * D], cm, sg, bt);
                        }
                        runs[2 * e] = sg; runs[2 * e + 1] = bt;
                    } else {
                        const int *x = d.xi + col;
                        long long S = ((long long *)runs)[e];
                        for (int t = 0; t < nw; ++t) S += glob(x)[(size_t)mem[t] * D];
                        ((long long *)runs)[e] = S;
                    }
                }
                __syncthreads();
                if (tid < N) before[tid] += lab_cnt[tid];
                __syncthreads();
            }
            if (kind == K_CATEGORICAL) {                            // the tile's levels, ascending, onto the running value
                __syncthreads();
                for (int e = tid; e < items; e += 256) {
                    const int qq = e % dq;
                    const int hi = min(Lt, glob(d.maxcol)[q0 + qq] - l0);
                    double val = runs[e];
                    for (int r = 0; r < hi; ++r) val += glob(d.lghtab)[2 * lev[e * Lt + r] + 1];
                    runs[e] = val;
                }
            }
            __syncthreads();
        }
        // calc_logmarginal of every item's cluster: gaussian_cluster.jl:68-83, categorical_cluster.jl:53-66, negbinom_cluster.jl:53-60
        for (int e = tid; e < items; e += 256) {
            const int o = e / dq, qq = e - o * dq, l = occ[o], cn = s_cn[l];
            double val;
            if (kind == K_GAUSSIAN) {
                const double a_n = ((double)cn / 2.0 + 0.5);
                val = (-a_n) * log(runs[2 * e + 1]) + glob(d.lmtab)[cn];
            } else if (kind == K_NEGBINOM) {
                const long long S = ((long long *)runs)[e];
                val = glob(d.lgtab)[S + 1] - glob(d.lgtab)[S + (cn + 1 + 1)] + glob(d.lgtab)[1 + cn];
            } else {
                val = runs[e];
            }
            lm[(size_t)(q0 + qq) * N + l] = val;
        }
        __syncthreads();
    }
}

// One lane per (chain of the batch, feature): src/pmdi.jl:357-367 without the coin
__global__ void __launch_bounds__(256) density_feature_kernel(const DensityArgs a, int c0, int chains)
{
    const int N = a.N, K = a.K;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)chains * a.sumD) return;
    const int g = (int)(idx % a.sumD), cb = (int)(idx / a.sumD), c = c0 + cb;
    int k = 0;
    for (int kk = 0; kk < K; ++kk) if (g >= a.ds[kk].flag_off) k = kk;
    const int *ord = a.ord + ((size_t)c * K + k) * N;
    const int nocc = a.nocc[(size_t)c * K + k];
    const double *lm = a.lm + ((size_t)(a.lm_all ? c : cb) * a.sumD + g) * N;
    double bf = a.fnull[g] + 0.0;                                   // :357
    double cl = 0.0;
    for (int j = 0; j < nocc; ++j) {                                // labels by first appearance (:358)
        const double v = lm[ord[j]];
        bf += v;                                                    // :365
        cl += v;
    }
    long long q = 0;
    if (bf - bf == 0.0) {                                           // finite
        const double pr = 1.0 - 1.0 / (exp(bf + 1.0));              // :367
        q = pr > 0.0 ? (long long)floor(pr * 1048576.0 + 0.5) : 0;
    }
    const size_t at = (size_t)c * a.sumD + g;
    a.bf[at] = bf; a.cl[at] = cl; a.q[at] = q;
}

// One wavefront per (chain, pair): the rows the two datasets give the same label
__global__ void __launch_bounds__(64) density_agree_kernel(const DensityArgs a)
{
    const int K = a.K, c = blockIdx.x / a.G, p = blockIdx.x - c * a.G, lane = threadIdx.x;
    int ka = 0, left = p;
    while (left >= K - 1 - ka) { left -= K - 1 - ka; ++ka; }
    const int kb = ka + 1 + left;
    const int *sa = a.s + ((size_t)c * K + ka) * a.n, *sb = a.s + ((size_t)c * K + kb) * a.n;
    long long cnt = 0;
    for (long long i0 = 0; i0 < a.n; i0 += 64) {
        const long long i = i0 + lane;
        cnt += __popcll(__ballot(i < a.n && sa[i] == sb[i]));
    }
    if (lane == 0) a.agree[(size_t)c * a.npairs + p] = cnt;
}

// One workgroup (a wave) per chain; lane 0 does the sequential work
__global__ void __launch_bounds__(64) density_chain_kernel(const DensityArgs a)
{
    __shared__ double W[64], conn[256], F[256], link[256], T[256], Zs[256], s_ll[PMDI_KMAX_I];
    const int K = a.K, N = a.N, tid = threadIdx.x, c = blockIdx.x;
    const unsigned full = (1u << K) - 1u;
    const double *Pi = a.Pi + (size_t)c * K * N;
    W[tid] = 0.0;
    if (tid < K) {                                                  // ll[k]: the dataset's features ascending
        const DsetDev &d = a.ds[tid];
        const unsigned char *fl = a.flags ? a.flags + (size_t)c * a.sumD + d.flag_off : nullptr;
        const double *cl = a.cl + (size_t)c * a.sumD + d.flag_off;
        const double *fn = a.fnull + d.flag_off;
        double ll = 0.0;
        for (int q = 0; q < d.D; ++q) {
            const double t = (fl ? fl[q] != 0 : true) ? cl[q] : -fn[q];
            ll = q == 0 ? t : ll + t;
        }
        s_ll[tid] = ll;
        a.tr_ll[((size_t)a.T * a.C + c) * K + tid] = ll;
    }
    compute_T(K, N, Pi, T, tid, 64);
    __syncthreads();
    if (tid != 0) return;
    if (K > 1) fill_W(K, a.Phi + (size_t)c * a.npairs, W);
    conn_all(full, W, conn, F, link);
    zs_all(full, conn, T, Zs);
    const double logZ = log(Zs[full]);
    a.logZ[c] = logZ;
    double lprior = 0.0;
    for (int k = 0; k < K; ++k) {
        const int *cn = a.cn + ((size_t)c * K + k) * N;
        for (int l = 0; l < N; ++l)
            if (cn[l] > 0) lprior += (double)cn[l] * log(Pi[k * N + l]);
    }
    for (int p = 0; p < a.G; ++p) lprior += (double)a.agree[(size_t)c * a.npairs + p] * log(1.0 + a.Phi[(size_t)c * a.npairs + p]);
    lprior -= (double)a.n * logZ;
    double lj = s_ll[0];
    for (int k = 1; k < K; ++k) lj = lj + s_ll[k];
    lj = lj + lprior;
    a.tr_lprior[(size_t)a.T * a.C + c] = lprior;
    a.tr_lj[(size_t)a.T * a.C + c] = lj;
    const bool wins = lj > a.best_val[c];                           // a tie keeps the earlier state; a NaN never wins
    if (wins) { a.best_val[c] = lj; a.best_t[c] = a.T; }
    a.take[c] = wins ? 1 : 0;
}

__global__ void __launch_bounds__(256) density_best_kernel(const DensityArgs a)
{
    const int c = blockIdx.y;
    if (!a.take[c]) return;
    const long long Kn = (long long)a.K * a.n, idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx < Kn) a.best_s[(size_t)c * Kn + idx] = (unsigned char)a.s[(size_t)c * Kn + idx];
}

// One owner lane per feature, the chains in ascending order
__global__ void __launch_bounds__(256) density_sums_kernel(const DensityArgs a)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= a.sumD) return;
    double s1 = a.bf_sum[g], s2 = a.bf_sq_sum[g];
    long long ps = a.p_sum[g], bad = a.bad[g];
    for (int c = 0; c < a.C; ++c) {
        const double bf = a.bf[(size_t)c * a.sumD + g];
        if (!(bf - bf == 0.0)) { bad += 1; continue; }
        s1 += bf;
        s2 += bf * bf;
        ps += a.q[(size_t)c * a.sumD + g];
    }
    a.bf_sum[g] = s1; a.bf_sq_sum[g] = s2; a.p_sum[g] = ps; a.bad[g] = bad;
}

__global__ void __launch_bounds__(256) density_clear_kernel(const DensityArgs a)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= a.C) return;
    a.best_val[c] = -__builtin_huge_val();
    a.best_t[c] = -1;
}

}  // namespace

hipError_t pmdi_launch_density_add(const DensityArgs &a, hipStream_t stream)
{
    const long long Kn = (long long)a.K * a.n;
    for (int c0 = 0; c0 < a.C; c0 += a.Cb) {
        const int chains = a.C - c0 < a.Cb ? a.C - c0 : a.Cb;
        hipLaunchKernelGGL(density_stats_kernel, dim3((unsigned)chains * a.K), dim3(256), DS_LDS, stream, a, c0);
        hipLaunchKernelGGL(density_feature_kernel, dim3((unsigned)(((long long)chains * a.sumD + 255) / 256)), dim3(256), 0, stream, a, c0, chains);
    }
    if (a.G > 0) hipLaunchKernelGGL(density_agree_kernel, dim3((unsigned)a.C * a.G), dim3(64), 0, stream, a);
    hipLaunchKernelGGL(density_chain_kernel, dim3((unsigned)a.C), dim3(64), 0, stream, a);
    hipLaunchKernelGGL(density_best_kernel, dim3((unsigned)((Kn + 255) / 256), (unsigned)a.C), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(density_sums_kernel, dim3((unsigned)((a.sumD + 255) / 256)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t pmdi_launch_density_clear(const DensityArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(density_clear_kernel, dim3((unsigned)((a.C + 255) / 256)), dim3(256), 0, stream, a);
    return hipGetLastError();
}
