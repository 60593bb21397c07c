// pmdi_predict_coupled.hip -- the Phi-coupled stage of a coupled add of the streaming predictive accumulator (include/pmdi_hip.h,
// pmdi_predict_*_coupled): the posterior of a new observation's labels c = (c_1 .. c_K) in one chain's state,
//     p(c | state) ~ prod_k Pi_k[c_k] f_k(x_k | cluster c_k) * prod_{a<b} (1 + Phi_ab [c_a == c_b]),
// summed over its N^K label combinations by the subset recursions of pmdi_subset.h.  Three kernels beside pmdi_predict.hip's:
//   predict_chain_tables_kernel    per (chain, table): conn of the chain's W, conn2 of every pair contracted, and log Z0 (g = Pi);
//                                  they depend on the chain only and are written once per add
//   predict_couple_kernel          per (chain of the batch, new row), one wave: g = exp(lp - mx) * Pi, T, Zs, the joint label
//                                  marginals qj, the pair probabilities fq and the joint log density incj
//   predict_coupled_reduce_kernel  fused_new and lpd_joint_sum, one lane per entry, chains in order
// sim_joint and new_cluster_joint come from pmdi_predict.hip's gather and reduce kernels pointed at qj.
// The subset tables are indexed by run-time masks: they live in LDS, never in private arrays.  Every entry of every table is one
// lane's work in the stated order, so no result depends on the mapping.  Compile with -ffp-contract=off.
#include "pmdi_device.h"
#include "pmdi_subset.h"

using namespace pmdi_dev;

namespace {

// pair p of Phi's order as (a, b), a < b
__device__ __forceinline__ void pair_of(int K, int p, int &ka, int &kb)
{
    int a = 0, left = p;
    while (left >= K - 1 - a) { left -= K - 1 - a; ++a; }
    ka = a; kb = a + 1 + left;
}

// One workgroup (a wave) per (chain, table): table 0 is conn_all(full, W) and Z0, table 1 + p is conn_all(full - b, W2) of pair p
__global__ void __launch_bounds__(64) predict_chain_tables_kernel(const PredictArgs a, const CoupledArgs cp)
{
    __shared__ double W[64], W2[64], conn[256], F[256], link[256], T[256], Zs[256];
    const int K = a.K, N = a.N, tid = threadIdx.x;
    const int tables = 1 + cp.npairs, nsub = cp.nsub;
    const int c = blockIdx.x / tables, t = blockIdx.x - c * tables;
    const unsigned full = (unsigned)nsub - 1u;
    W[tid] = 0.0;
    for (int e = tid; e < nsub; e += 64) conn[e] = 0.0;              // (entries outside the active set: written as zeros, never read)
    __syncthreads();
    if (tid == 0) {
        fill_W(K, cp.Phi + (size_t)c * cp.npairs, W);
        if (t == 0) {
            conn_all(full, W, conn, F, link);
        } else {
            int ka, kb;
            pair_of(K, t - 1, ka, kb);
            contract_W(K, ka, kb, W, W2);
            conn_all(full ^ (1u << kb), W2, conn, F, link);
        }
    }
    __syncthreads();
    double *out = cp.conn + ((size_t)c * tables + t) * nsub;
    for (int e = tid; e < nsub; e += 64) out[e] = conn[e];
    if (t != 0) return;
    compute_T(K, N, a.Pi + (size_t)c * K * N, T, tid, 64);
    __syncthreads();
    if (tid == 0) {
        zs_all(full, conn, T, Zs);
        const double Z0 = Zs[full];
        cp.Z0[c] = Z0;
        cp.logZ0[c] = log(Z0);
    }
}

// One workgroup (a wave) per (chain of the batch, new row).  LDS: g [K][N], T [nsub], Zs [nsub], mx [8] doubles, then 8 ints.
__global__ void __launch_bounds__(64) predict_couple_kernel(const PredictArgs a, const CoupledArgs cp, int c0)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int K = a.K, N = a.N, G = cp.npairs, nsub = cp.nsub, tid = threadIdx.x;
    const long long m = a.m;
    const int cb = (int)(blockIdx.x / m), c = c0 + cb;
    const long long j = blockIdx.x - (long long)cb * m;
    double *g = (double *)smem, *T = g + K * N, *Zs = T + nsub, *mxs = Zs + nsub;
    int *qn = (int *)(mxs + 8);
    const unsigned full = (unsigned)nsub - 1u;
    const double *Pi = a.Pi + (size_t)c * K * N;
    const double *conn = cp.conn + (size_t)c * (1 + G) * nsub;
    const size_t lp_chain = (size_t)(a.lp_all ? c : cb);

    // step 1: mx_k and g[k][l] = exp(lp_l - mx_k) * Pi[k][l]
    for (int k = 0; k < K; ++k) {
        const double *lp = a.lp + ((lp_chain * K + k) * m + j) * N;
        double v = -INFINITY;
        for (int l = tid; l < N; l += 64) { const double x = lp[l]; v = (x > v) ? x : v; }
        const double mx = wave_max_f64(v);
        if (tid == 0) mxs[k] = mx;
        for (int l = tid; l < N; l += 64) {
            const double f = exp(lp[l] - mx) * Pi[k * N + l];
            g[k * N + l] = f;
            if (cp.g) cp.g[(((size_t)c * K + k) * m + j) * N + l] = f;
        }
    }
    if (tid < 8) qn[tid] = 0;
    if (tid == 0) Zs[0] = 1.0;
    __syncthreads();
    // step 2
    compute_T(K, N, g, T, tid, 64);
    __syncthreads();
    // step 3: Zs by the size of the subset; every entry reads smaller subsets only
    for (int size = 1; size <= K; ++size) {
        for (unsigned S = 1 + tid; S < (unsigned)nsub; S += 64)
            if (__popc(S) == size) Zs[S] = zs_one(S, conn, T, Zs);
        __syncthreads();
    }
    const double Z = Zs[full];
    const bool ok = Z > 0.0 && Z <= 1.7976931348623157e308;         // (Z = 0 or not finite: no weight anywhere)
    // step 4: the joint marginal of every (dataset, label)
    for (int e = tid; e < K * N; e += 64) {
        const int k = e / N, l = e - k * N;
        const double S = marginal_sum(K, N, k, l, full ^ (1u << k), conn, g, Zs);
        const double wj = S / Z;
        const int qv = ok ? (int)floor(wj * 1048576.0 + 0.5) : 0;
        cp.qj[(((size_t)c * K + k) * m + j) * N + l] = qv;
        if (qv && a.cn[((size_t)c * K + k) * N + l] == 0) atomicAdd(&qn[k], qv);
    }
    // step 5: the probability that a and b give the row one label
    for (int p = tid; p < G; p += 64) {
        int ka, kb;
        pair_of(K, p, ka, kb);
        const double R = pair_sum(ka, kb, full ^ (1u << ka) ^ (1u << kb), conn + (size_t)(1 + p) * nsub, T, Zs) *
                         (1.0 + cp.Phi[(size_t)c * G + p]);
        const double w = R / Z;
        cp.fq[((size_t)c * G + p) * m + j] = ok ? (int)floor(w * 1048576.0 + 0.5) : 0;
    }
    // step 6: the joint log predictive density
    if (tid == 0) {
        double smx = mxs[0];
        for (int k = 1; k < K; ++k) smx = smx + mxs[k];
        cp.incj[(size_t)c * m + j] = (log(Z) - cp.logZ0[c]) + smx;
        if (cp.Z) cp.Z[(size_t)c * m + j] = Z;
    }
    __syncthreads();
    if (tid < K) cp.qjnew[((size_t)c * K + tid) * m + j] = qn[tid];
}

// One lane per entry of fused_new [G][m], then of lpd_joint_sum [m]; chains in order
__global__ void __launch_bounds__(256) predict_coupled_reduce_kernel(const PredictArgs a, const CoupledArgs cp)
{
    const long long Gm = (long long)cp.npairs * a.m;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx < Gm) {
        long long f = cp.fused_new[idx];
        for (int c = 0; c < a.C; ++c) f += cp.fq[(size_t)c * Gm + idx];
        cp.fused_new[idx] = f;
    } else if (idx < Gm + a.m) {
        const long long j = idx - Gm;
        double lpd = cp.lpd_joint_sum[j];
        for (int c = 0; c < a.C; ++c) lpd = lpd + cp.incj[(size_t)c * a.m + j];
        cp.lpd_joint_sum[j] = lpd;
    }
}

__global__ void __launch_bounds__(256) predict_coupled_merge_kernel(const PredictArgs a, const CoupledArgs cp, const long long *__restrict__ fused_b,
                                                                    const double *__restrict__ lpdj_b)
{
    const long long Gm = (long long)cp.npairs * a.m;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx < Gm) cp.fused_new[idx] += fused_b[idx];
    else if (idx < Gm + a.m) cp.lpd_joint_sum[idx - Gm] = cp.lpd_joint_sum[idx - Gm] + lpdj_b[idx - Gm];
}

}  // namespace

void pmdi_launch_predict_chain_tables(const PredictArgs &a, const CoupledArgs &cp, hipStream_t stream)
{
    hipLaunchKernelGGL(predict_chain_tables_kernel, dim3((unsigned)a.C * (1 + cp.npairs)), dim3(64), 0, stream, a, cp);
}

void pmdi_launch_predict_couple(const PredictArgs &a, const CoupledArgs &cp, int c0, int chains, hipStream_t stream)
{
    const size_t lds = ((size_t)a.K * a.N + 2 * (size_t)cp.nsub + 8) * 8 + 8 * 4;      // at most 8 x 255 + 512 + 8 doubles: 20.5 KiB
    hipLaunchKernelGGL(predict_couple_kernel, dim3((unsigned)((long long)chains * a.m)), dim3(64), lds, stream, a, cp, c0);
}

void pmdi_launch_predict_coupled_reduce(const PredictArgs &a, const CoupledArgs &cp, hipStream_t stream)
{
    const long long lanes = ((long long)cp.npairs + 1) * a.m;
    hipLaunchKernelGGL(predict_coupled_reduce_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, stream, a, cp);
}

hipError_t pmdi_launch_predict_coupled_merge(const PredictArgs &a, const CoupledArgs &cp, const long long *fused_b, const double *lpdj_b, hipStream_t stream)
{
    const long long lanes = ((long long)cp.npairs + 1) * a.m;
    hipLaunchKernelGGL(predict_coupled_merge_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, stream, a, cp, fused_b, lpdj_b);
    return hipGetLastError();
}
