// pmdi_predict.hip -- one add of the streaming predictive accumulator (include/pmdi_hip.h, pmdi_predict_*): where do m held-out
// rows fall in the current state of every chain?  Four kernels per add, five with imputation:
//   predict_weights_kernel    per (chain, dataset, label): the label's cluster rebuilt from its members in ascending observation
//                             order under the chain's feature flags (what featsel_label_kernel does with every flag on), then
//                             calc_logprob of every new row against it, features in ascending order (cluster_logprob_kernel's sums)
//   predict_normalise_kernel  per (chain, dataset, new row): the sweep's proposal over the N labels (src/pmdi.jl:231-248 without
//                             Phi) as fixed-point weights q, its log increment, and the weight on the sample's empty labels
//   predict_gather_kernel     sim[k][j][i] += sum over the chains of q[c][k][j][s[c][k][i]]: the hot path, exact integers
//   predict_reduce_kernel     new_cluster and lpd_sum, one lane per (dataset, new row), chains in order
//   predict_impute_kernel     (accumulators with imputation) loc_sum[j][f] += sum over the chains of sum_l q[c][k][j][l] * mu[c][k][l][f],
//                             per batch of chains after its normalise kernel, and once more with the joint weights of a coupled add
// A coupled add (pmdi_predict_coupled.hip) runs its coupling kernel after every batch's normalise kernel and sends its joint weights
// through the same gather and reduce kernels (launch_sums).
// The arithmetic is pmdi_arith.h's and the tables are the host-built ones, so the integer kinds agree with a CPU evaluation bit for
// bit.  Compile with -ffp-contract=off.
#include "pmdi_device.h"

using namespace pmdi_dev;

namespace {

constexpr int PW_CHUNK = 4096;              // observations whose members are listed per pass ...
constexpr int PW_SEG = PW_CHUNK / 4;        // ... a quarter per wave, so the list keeps the observation order without a block-wide scan
constexpr int PW_TILE_INTS = 10240;         // at most 40 KiB beside the list: categorical level counts of a tile of features (the launcher sizes it)
constexpr int PG_OB = 512;                  // gather tile: observations (two per lane) ...
constexpr int PG_JS = 32;                   // ... times new rows (accumulators per observation)
constexpr int PG_ROW = PG_JS + 4;           // LDS row stride in dwords: one 16-byte access of padding, rows start 16-byte aligned
constexpr int PG_WINDOW = 2047;             // chains whose q (<= 2^20 each) one int32 accumulator takes
constexpr int PI_F = 64;                    // impute tile: features (one per lane of a wave) ...
constexpr int PI_R = 2;                     // ... times new rows per lane, ...
constexpr int PI_J = 4 * PI_R;              // ... four waves of them
constexpr int PI_LC = 32;                   // labels per stage of the impute kernel
constexpr int PI_MU = PI_LC / 4;            // mu values a lane stages (its feature, every fourth label from its wave's index)
static_assert(PI_J * PI_LC == 256, "one staged q entry per lane");

// MASKED (pmdi_predict_create_masked): a feature of new row j counts only where obs[k][j][f] is set, the leading term becomes
// per row, and the Gaussian locations go to a.mu for the imputation sums.  The other instantiation is the code it always was.
template <bool MASKED>
__global__ void __launch_bounds__(256) predict_weights_kernel(const PredictArgs a, int c0)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int *list = (int *)smem;                                        // [4][PW_SEG] members of the chunk, per wave in ascending order
    int *tile = (int *)(smem + (size_t)PW_CHUNK * 4);               // [ltile][L] level counts | double2 [256] (mu, lambda) | int64 [256] Sigma
    __shared__ int s_count, wcount[4];
    __shared__ double s_start;
    const int N = a.N, K = a.K;
    const long long n = a.n, m = a.m;
    const int l = blockIdx.x % N;
    const int k = (blockIdx.x / N) % K;
    const int cb = blockIdx.x / (N * K), c = c0 + cb;
    const DsetDev &d = a.ds[k];
    const int D = d.D, L = d.L, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int *traj = a.s + ((size_t)c * K + k) * n;
    const unsigned char *fl = a.flags ? a.flags + (size_t)c * a.sumD + d.flag_off : nullptr;
    double *lp = a.lp + (((size_t)(a.lp_all ? c : cb) * K + k) * m) * N + l;      // this label's column: stride N over the new rows
    const double *nxf = a.nxf[k];
    const int *nxi = a.nxi[k];
    const unsigned char *ob = nullptr;                              // [m][D], null: every entry of the dataset is observed
    if constexpr (MASKED) ob = a.obs[k];

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

    // what calc_logprob starts from, before its loop over the features: the same for every new row, so one lane forms it (the
    // categorical sum in feature order) and the workgroup reads it back
    if (MASKED && ob) {                                             // per row: the features that are on and observed
        const double gt = d.kind == K_GAUSSIAN ? glob(d.gtab)[cn] : 0.0;
        for (long long j = tid; j < m; j += 256) {
            const unsigned char *oj = ob + (size_t)j * D;
            double start = 0.0;
            if (d.kind == K_GAUSSIAN) {
                int nobs = 0;
                for (int q = 0; q < D; ++q) nobs += ((fl ? fl[q] != 0 : true) && oj[q] != 0);
                start = (double)nobs * gt;
            } else if (d.kind == K_CATEGORICAL) {
                double acc = 0.0;
                for (int q = 0; q < D; ++q) {
                    if ((fl && !fl[q]) || !oj[q]) continue;
                    acc += glob(d.lhtab)[glob(d.maxcol)[q] + 2 * cn];
                }
                start = -acc;
            }
            lp[(size_t)j * N] = start;
        }
    } else {
        if (tid == 0) {
            double start = 0.0;
            if (d.kind == K_GAUSSIAN) {
                int nflag = 0;
                for (int q = 0; q < D; ++q) nflag += (fl ? fl[q] != 0 : 1);
                start = (double)nflag * glob(d.gtab)[cn];
            } else if (d.kind == K_CATEGORICAL) {
                double acc = 0.0;
                for (int q = 0; q < D; ++q) {
                    if (fl && !fl[q]) continue;
                    acc += glob(d.lhtab)[glob(d.maxcol)[q] + 2 * cn];
                }
                start = -acc;
            }
            s_start = start;
        }
        __syncthreads();
        const double start = s_start;
        for (long long j = tid; j < m; j += 256) lp[(size_t)j * N] = start;
    }

    // tiles of features in ascending order: rebuild the tile's statistics from the members, park them in LDS, add the tile's terms
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
            for (long long base = 0; base < n; base += PW_CHUNK) {
                int wc = 0;
                const long long seg = base + (long long)wave * PW_SEG;
                for (int st = 0; st < PW_SEG; st += 64) {
                    const long long i = seg + st + lane;
                    const bool f = i < n && traj[i] == l;
                    const unsigned long long b = __ballot(f);
                    if (f) list[wave * PW_SEG + wc + __popcll(b & below)] = (int)i;
                    wc += __popcll(b);
                }
                if (lane == 0) wcount[wave] = wc;
                __syncthreads();
                for (int w = 0; w < 4; ++w) {
                    const int nw = wcount[w];
                    const int *mem = list + w * PW_SEG;
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
            if (tid < dq) {
                double mu, lam;
                pmdi_arith::gauss_ml(cn, sg, bt, mu, lam);
                ((double2 *)tile)[tid] = make_double2(mu, lam);
                if constexpr (MASKED)
                    if (a.mu) a.mu[((((size_t)(a.lp_all ? c : cb) * K + k) * N + l) * a.Dmax) + q] = mu;
            }
        } else if (d.kind == K_NEGBINOM) {
            if (tid < dq) ((long long *)tile)[tid] = S;
        }
        __syncthreads();
        for (long long j = tid; j < m; j += 256) {
            double out = lp[(size_t)j * N];
            for (int qq = 0; qq < dq; ++qq) {
                const int f = q0 + qq;
                if (fl && !fl[f]) continue;
                if constexpr (MASKED)
                    if (ob && !ob[(size_t)j * D + f]) continue;     // (before the entry is read: it may be anything)
                if (d.kind == K_GAUSSIAN) {
                    double ta, tb;
                    gauss_terms(glob(nxf)[(size_t)j * D + f], (double)cn, ((const double2 *)tile)[qq], ta, tb);
                    out += ta; out -= tb;
                } else if (d.kind == K_CATEGORICAL) {
                    const int cnt = tile[qq * L + (glob(nxi)[(size_t)j * D + f] - 1)];
                    out += (cn == 0) ? glob(d.lhtab)[1] : glob(d.lhtab)[2 * cnt + 1];
                } else {
                    out += negbin_term(glob(d.lgtab), cn, glob(nxi)[(size_t)j * D + f], ((const long long *)tile)[qq]);
                }
            }
            lp[(size_t)j * N] = out;
        }
        __syncthreads();
    }
}

// One lane per (chain of the batch, dataset, new row): src/pmdi.jl:231-248 over the N labels, without Phi
__global__ void __launch_bounds__(256) predict_normalise_kernel(const PredictArgs a, int c0, int chains)
{
    const int N = a.N, K = a.K;
    const long long m = a.m;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)chains * K * m) return;
    const long long j = idx % m;
    const int k = (int)((idx / m) % K), cb = (int)(idx / (m * K)), c = c0 + cb;
    const double *lp = a.lp + ((((size_t)(a.lp_all ? c : cb) * K + k) * m) + j) * N;
    const double *Pi = a.Pi + ((size_t)c * K + k) * N;
    const int *cn = a.cn + ((size_t)c * K + k) * N;
    const size_t row = ((size_t)c * K + k) * m + j;
    int *q = a.q + row * N;
    double mx = lp[0];
    for (int l = 1; l < N; ++l) { const double v = lp[l]; mx = (v > mx) ? v : mx; }
    double F = exp(lp[0] - mx) * Pi[0];
    for (int l = 1; l < N; ++l) F = F + exp(lp[l] - mx) * Pi[l];
    a.inc[row] = log(F) + mx;
    int qn = 0;
    for (int l = 0; l < N; ++l) {
        const double f = exp(lp[l] - mx) * Pi[l];
        const double w = f / F;
        const int qv = (F > 0.0 && F <= 1.7976931348623157e308) ? (int)floor(w * 1048576.0 + 0.5) : 0;      // (F = 0 or not finite: no weight anywhere)
        q[l] = qv;
        if (cn[l] == 0) qn += qv;
    }
    a.qnew[row] = qn;
}

// sim[k][j][i] += sum_c q[c][k][j][s[c][k][i]].  A workgroup owns PG_OB observations x PG_JS new rows of one dataset: two
// observations per lane, PG_JS int32 accumulators each.  Per chain it stages q[c][k][strip][0..N) in LDS transposed to [label][row]
// (row N stays zero: labels outside 0..N-1 and the lanes past n read it), and every lane adds the row of its label with 16-byte LDS
// reads.  nbuf = 2: the staging alternates between two buffers, one barrier per chain.  Every entry of sim has one owner: no atomics.
__global__ void __launch_bounds__(256) predict_gather_kernel(const PredictArgs a, int nbuf)
{
    extern __shared__ __attribute__((aligned(16))) int qs[];        // [nbuf][N + 1][PG_ROW]
    const int N = a.N, K = a.K, C = a.C, tid = threadIdx.x;
    const long long n = a.n, m = a.m;
    const int k = blockIdx.z;
    const long long j0 = (long long)blockIdx.y * PG_JS;
    const long long i0 = (long long)blockIdx.x * PG_OB + tid, i1 = i0 + 256;
    const int jn = (int)min((long long)PG_JS, m - j0);
    const int bufsz = (N + 1) * PG_ROW;
    for (int e = tid; e < nbuf * bufsz; e += 256) qs[e] = 0;
    __syncthreads();
    int acc0[PG_JS], acc1[PG_JS];
#pragma unroll
    for (int t = 0; t < PG_JS; ++t) { acc0[t] = 0; acc1[t] = 0; }
    auto flush = [&]() {
        int zero = 0;
        // The opaque zero keeps the compiler from forming the 64 row addresses ahead of the chain loop and holding them in
        // registers across it: this build has 162 VGPRs (3 waves per SIMD) with it and 234 (2 waves) without, no spills either way.
        // Only occupancy rests on it, no result; tests/test_predict_host.py keeps an eye on the register count.
        asm volatile("" : "+s"(zero));
        long long *row = a.sim + ((size_t)k * m + j0) * n + zero;
#pragma unroll
        for (int t = 0; t < PG_JS; ++t) {
            if (t < jn) {
                if (i0 < n) row[i0] += acc0[t];
                if (i1 < n) row[i1] += acc1[t];
            }
            row += n;
            acc0[t] = 0; acc1[t] = 0;
        }
    };
    int window = 0;
    for (int c = 0; c < C; ++c) {
        int *buf = qs + (nbuf == 2 ? (c & 1) * bufsz : 0);
        if (nbuf == 1) __syncthreads();                             // the last chain's reads are done
        const int *src = a.q + (((size_t)c * K + k) * m + j0) * N;  // the strip's rows are contiguous: [row][label]
        for (int e = tid; e < jn * N; e += 256) {
            const int j = e / N, l = e - j * N;
            buf[l * PG_ROW + j] = src[e];
        }
        const int *sr = a.s + ((size_t)c * K + k) * n;
        const int v0 = i0 < n ? sr[i0] : N, v1 = i1 < n ? sr[i1] : N;
        const int r0 = (unsigned)v0 < (unsigned)N ? v0 : N, r1 = (unsigned)v1 < (unsigned)N ? v1 : N;
        __syncthreads();
        const int4 *p0 = (const int4 *)(buf + r0 * PG_ROW), *p1 = (const int4 *)(buf + r1 * PG_ROW);
#pragma unroll
        for (int t = 0; t < PG_JS / 4; ++t) {
            const int4 x = p0[t], y = p1[t];
            acc0[4 * t] += x.x; acc0[4 * t + 1] += x.y; acc0[4 * t + 2] += x.z; acc0[4 * t + 3] += x.w;
            acc1[4 * t] += y.x; acc1[4 * t + 1] += y.y; acc1[4 * t + 2] += y.z; acc1[4 * t + 3] += y.w;
        }
        if (++window == PG_WINDOW) { flush(); window = 0; }
    }
    if (window) flush();
}

// One lane per (dataset, new row), chains in order: the integer sum is exact, lpd_sum = ((lpd_sum + inc_0) + inc_1) + ...
// (inc null: the joint sums of a coupled add, whose log density has one entry per new row and its own reduce)
__global__ void __launch_bounds__(256) predict_reduce_kernel(const PredictArgs a)
{
    const long long Km = (long long)a.K * a.m;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= Km) return;
    long long nc = a.new_cluster[idx];
    if (!a.inc) {
        for (int c = 0; c < a.C; ++c) nc += a.qnew[(size_t)c * Km + idx];
        a.new_cluster[idx] = nc;
        return;
    }
    double lpd = a.lpd_sum[idx];
    for (int c = 0; c < a.C; ++c) {
        nc += a.qnew[(size_t)c * Km + idx];
        lpd = lpd + a.inc[(size_t)c * Km + idx];
    }
    a.new_cluster[idx] = nc;
    a.lpd_sum[idx] = lpd;
}

__global__ void __launch_bounds__(256) predict_merge_kernel(const PredictArgs a, const long long *__restrict__ sim_b,
                                                            const long long *__restrict__ nc_b, const double *__restrict__ lpd_b)
{
    const long long Km = (long long)a.K * a.m, total = Km * a.n;
    const long long t0 = (long long)blockIdx.x * 256 + threadIdx.x, step = (long long)gridDim.x * 256;
    for (long long e = t0; e < total; e += step) a.sim[e] += sim_b[e];
    for (long long e = t0; e < Km; e += step) {
        a.new_cluster[e] += nc_b[e];
        if (lpd_b) a.lpd_sum[e] = a.lpd_sum[e] + lpd_b[e];
    }
}

// loc[j][off_k + f] += sum over the batch's chains (ascending, where the chain has the feature on) of
//     e = ((0 + q[c][k][j][0] * mu[c][k][0][f]) + q[c][k][j][1] * mu[c][k][1][f]) + ...       labels ascending, separate multiply and add
// for the Gaussian datasets.  A workgroup owns PI_J new rows x PI_F features of one dataset: a lane one feature (its wave's lane
// index) and PI_R rows (its wave's).  A stage is PI_LC labels of one chain: mu [label][feature] and q transposed to [label][row] go
// through registers into one of two LDS buffers -- the next stage's global reads are in flight while this one is summed, one
// barrier per stage.  The mu row is read with one conflict-free 8-byte access per lane, the q of the wave's rows with one
// broadcast.  e and the running sums live in registers across the stages, so no value depends on PI_LC or the tile; every entry
// of loc has one owner: no atomics.  count: the owners of row tile 0 also add the chains with the feature on to flag_on.
__global__ void __launch_bounds__(256) predict_impute_kernel(const PredictArgs a, const int *__restrict__ qsrc, double *__restrict__ loc,
                                                             int c0, int chains, int count)
{
    __shared__ __attribute__((aligned(16))) double mus[2][PI_LC][PI_F];
    __shared__ __attribute__((aligned(16))) int qs[2][PI_LC][PI_J];
    const int k = blockIdx.z;
    const DsetDev &d = a.ds[k];
    const int D = d.D, N = a.N, K = a.K, Dmax = a.Dmax;
    const int f0 = blockIdx.y * PI_F;
    if (d.kind != K_GAUSSIAN || f0 >= D) return;                    // (the grid spans the largest Gaussian D; uniform per workgroup)
    const long long m = a.m, j0 = (long long)blockIdx.x * PI_J;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = f0 + lane;
    const long long jr = j0 + wave * PI_R;
    const bool mine = f < D;
    double acc[PI_R];
#pragma unroll
    for (int r = 0; r < PI_R; ++r) acc[r] = (mine && jr + r < m) ? loc[(size_t)(jr + r) * a.sumD + d.flag_off + f] : 0.0;
    const int nchunk = (N + PI_LC - 1) / PI_LC;
    const long long stages = (long long)chains * nchunk;
    const int ql = tid & (PI_LC - 1), qj = tid / PI_LC;             // the q entry this lane stages: label of the chunk, row of the tile
    double pm[PI_MU];
    int pq = 0;
    auto fetch = [&](long long t) {
        const int cb = (int)(t / nchunk), l0 = (int)(t - (long long)cb * nchunk) * PI_LC, c = c0 + cb;
        const double *mu = a.mu + ((((size_t)(a.lp_all ? c : cb) * K + k) * N + l0) * Dmax) + f;
#pragma unroll
        for (int i = 0; i < PI_MU; ++i) {
            const int ll = wave + 4 * i;
            pm[i] = (mine && l0 + ll < N) ? mu[(size_t)ll * Dmax] : 0.0;
        }
        pq = (l0 + ql < N && j0 + qj < m) ? qsrc[((((size_t)c * K + k) * m + j0 + qj) * N) + l0 + ql] : 0;
    };
    if (stages > 0) fetch(0);
    long long fon = 0;
    double e[PI_R];
    for (long long t = 0; t < stages; ++t) {
        const int cb = (int)(t / nchunk), chunk = (int)(t - (long long)cb * nchunk), l0 = chunk * PI_LC;
        const int lc = min(PI_LC, N - l0), buf = (int)(t & 1);
#pragma unroll
        for (int i = 0; i < PI_MU; ++i) mus[buf][wave + 4 * i][lane] = pm[i];
        qs[buf][ql][qj] = pq;
        __syncthreads();                                            // (the buffer's last readers, two stages back, passed the barrier between)
        if (t + 1 < stages) fetch(t + 1);
        if (chunk == 0) {
#pragma unroll
            for (int r = 0; r < PI_R; ++r) e[r] = 0.0;
        }
        for (int ll = 0; ll < lc; ++ll) {
            const double u = mus[buf][ll][lane];
#pragma unroll
            for (int r = 0; r < PI_R; ++r) e[r] = e[r] + (double)qs[buf][ll][wave * PI_R + r] * u;
        }
        if (chunk == nchunk - 1) {
            const bool on = mine && (a.flags ? a.flags[(size_t)(c0 + cb) * a.sumD + d.flag_off + f] != 0 : true);
            fon += on;
            if (on) {
#pragma unroll
                for (int r = 0; r < PI_R; ++r) acc[r] = acc[r] + e[r];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < PI_R; ++r)
        if (mine && jr + r < m) loc[(size_t)(jr + r) * a.sumD + d.flag_off + f] = acc[r];
    if (count && blockIdx.x == 0 && wave == 0 && mine) a.flag_on[d.flag_off + f] += fon;
}

__global__ void __launch_bounds__(256) predict_merge_imputed_kernel(const PredictArgs a, const double *__restrict__ loc_b,
                                                                    const double *__restrict__ locj_b, const long long *__restrict__ flag_b)
{
    const long long total = a.m * a.sumD;
    const long long t0 = (long long)blockIdx.x * 256 + threadIdx.x, step = (long long)gridDim.x * 256;
    for (long long e = t0; e < total; e += step) {
        a.loc_sum[e] = a.loc_sum[e] + loc_b[e];
        if (locj_b) a.loc_joint_sum[e] = a.loc_joint_sum[e] + locj_b[e];
    }
    for (long long e = t0; e < a.sumD; e += step) a.flag_on[e] += flag_b[e];
}

// The imputation sums of one batch of chains from the weights qsrc (q, or the joint qj) into loc
void launch_impute(const PredictArgs &b, const int *qsrc, double *loc, int c0, int chains, int count, hipStream_t stream)
{
    int Dg = 0;
    for (int k = 0; k < b.K; ++k)
        if (b.ds[k].kind == K_GAUSSIAN && b.ds[k].D > Dg) Dg = b.ds[k].D;
    if (Dg == 0) return;
    dim3 grid((unsigned)((b.m + PI_J - 1) / PI_J), (unsigned)((Dg + PI_F - 1) / PI_F), (unsigned)b.K);
    hipLaunchKernelGGL(predict_impute_kernel, grid, dim3(256), 0, stream, b, qsrc, loc, c0, chains, count);
}

// The sums of one add from its weights: sim += the gather of a.q over a.s, new_cluster += a.qnew and lpd_sum + a.inc in chain
// order.  A coupled add calls it twice: with the per-dataset buffers, then with q, qnew, sim, new_cluster pointed at the joint ones.
void launch_sums(const PredictArgs &b, hipStream_t stream)
{
    const size_t buf = (size_t)(b.N + 1) * PG_ROW * 4;
    const int nbuf = 2 * buf <= 48 * 1024 ? 2 : 1;
    dim3 grid((unsigned)((b.n + PG_OB - 1) / PG_OB), (unsigned)((b.m + PG_JS - 1) / PG_JS), (unsigned)b.K);
    hipLaunchKernelGGL(predict_gather_kernel, grid, dim3(256), nbuf * buf, stream, b, nbuf);
    hipLaunchKernelGGL(predict_reduce_kernel, dim3((unsigned)(((long long)b.K * b.m + 255) / 256)), dim3(256), 0, stream, b);
}

}  // namespace

hipError_t pmdi_launch_predict_add(const PredictArgs &a, hipStream_t stream, const CoupledArgs *cp)
{
    PredictArgs b = a;
    int Lmax = 1;
    for (int k = 0; k < a.K; ++k)
        if (a.ds[k].kind == K_CATEGORICAL && a.ds[k].L > Lmax) Lmax = a.ds[k].L;
    b.ltile = PW_TILE_INTS / Lmax;                                  // L <= 4096 (pmdi_create): at least two features per tile
    if (b.ltile > 256) b.ltile = 256;
    // beside the member list: the parked statistics of 256 features (16 bytes each), or a categorical tile's level counts
    size_t tile_bytes = 256 * 16;
    for (int k = 0; k < a.K; ++k)
        if (a.ds[k].kind == K_CATEGORICAL) {
            const size_t need = (size_t)(a.ds[k].D < b.ltile ? a.ds[k].D : b.ltile) * a.ds[k].L * 4;
            if (need > tile_bytes) tile_bytes = need;
        }
    const size_t lds_w = (size_t)PW_CHUNK * 4 + ((tile_bytes + 15) & ~(size_t)15);
    if (cp) pmdi_launch_predict_chain_tables(b, *cp, stream);
    for (int c0 = 0; c0 < a.C; c0 += a.Cb) {
        const int chains = a.C - c0 < a.Cb ? a.C - c0 : a.Cb;
        if (a.masked) hipLaunchKernelGGL(predict_weights_kernel<true>, dim3((unsigned)chains * a.K * a.N), dim3(256), lds_w, stream, b, c0);
        else hipLaunchKernelGGL(predict_weights_kernel<false>, dim3((unsigned)chains * a.K * a.N), dim3(256), lds_w, stream, b, c0);
        const long long rows = (long long)chains * a.K * a.m;
        hipLaunchKernelGGL(predict_normalise_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, b, c0, chains);
        if (a.loc_sum) launch_impute(b, b.q, b.loc_sum, c0, chains, 1, stream);      // (while the batch's mu is live)
        if (cp) pmdi_launch_predict_couple(b, *cp, c0, chains, stream);      // (while the batch's lp is live)
        if (cp && a.loc_joint_sum) launch_impute(b, cp->qj, b.loc_joint_sum, c0, chains, 0, stream);
    }
    launch_sums(b, stream);
    if (cp) {
        PredictArgs j = b;
        j.q = cp->qj; j.qnew = cp->qjnew; j.inc = nullptr;
        j.sim = cp->sim_joint; j.new_cluster = cp->new_cluster_joint; j.lpd_sum = nullptr;
        launch_sums(j, stream);
        pmdi_launch_predict_coupled_reduce(b, *cp, stream);
    }
    return hipGetLastError();
}

hipError_t pmdi_launch_predict_merge_imputed(const PredictArgs &a, const double *loc_b, const double *locj_b, const long long *flag_b, hipStream_t stream)
{
    long long grid = (a.m * a.sumD + 255) / 256;
    if (grid > 65536) grid = 65536;
    hipLaunchKernelGGL(predict_merge_imputed_kernel, dim3((unsigned)grid), dim3(256), 0, stream, a, loc_b, locj_b, flag_b);
    return hipGetLastError();
}

hipError_t pmdi_launch_predict_merge(const PredictArgs &a, const long long *sim_b, const long long *nc_b, const double *lpd_b, hipStream_t stream)
{
    const long long total = (long long)a.K * a.m * a.n;
    long long grid = (total + 255) / 256;
    if (grid > 65536) grid = 65536;
    hipLaunchKernelGGL(predict_merge_kernel, dim3((unsigned)grid), dim3(256), 0, stream, a, sim_b, nc_b, lpd_b);
    return hipGetLastError();
}
