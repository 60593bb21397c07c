// pmdi_summary.hip -- the streaming summary accumulator (include/pmdi_hip.h, pmdi_summary_*): what the reference's users read
// from the output file after a run (src/output_analysis/phi_plots.jl get_phi, nclust_plots.jl get_nclust,
// feature_select_plots.jl get_feature_select_probs) plus the per-chain moments behind R-hat, taken from every retained
// iteration of every chain on the device.  One add is four small launches on the accumulator's stream:
//   summary_nclust_kernel   the one kernel that touches real data: the number of distinct labels of every (chain, dataset) row
//   summary_welford_kernel  one lane per (chain, scalar): the Welford recurrences of M and Phi, separate IEEE operations
//   summary_pool_kernel     what is pooled over chains: histogram and per-chain integer sums of the cluster counts, and the trace
//                           row (sums over chains in chain order, one lane per scalar)
//   summary_flags_kernel    flag_count += feature flags (only when the source has feature selection on)
// The launches of one accumulator are ordered on one stream; every word of the state but flag_count (integer atomics) is
// owned by one lane of a launch, so the state is bit-defined by the order of the adds.
#include <hip/hip_runtime.h>

#include "pmdi_internal.h"

#pragma clang fp contract(off)      // the recurrences are defined with separate multiplies and adds (the build passes -ffp-contract=off too)

namespace {

typedef int sm_v4i __attribute__((ext_vector_type(4)));

// presence mask of the labels 0..32 NW - 1, NW words per lane, indexed by constants only (registers, no scratch).  A label
// outside 0..N-1 is not marked (the count stays <= N: it indexes the histogram) and raises `bad`.
template <int NW>
__device__ __forceinline__ void sm_mark(unsigned (&m)[NW], int v, unsigned N, unsigned &bad)
{
    const unsigned u = (unsigned)v;                          // a negative label is a large one
    const bool ok = u < N;
    bad |= ok ? 0u : 1u;
    const unsigned bit = ok ? (1u << (u & 31u)) : 0u;
    if (NW == 1) {
        m[0] |= bit;
    } else {
        const unsigned w = u >> 5;
#pragma unroll
        for (int i = 0; i < NW; ++i) m[i] |= (w == (unsigned)i) ? bit : 0u;
    }
}

template <int NW>
__device__ __forceinline__ void sm_mark4(unsigned (&m)[NW], sm_v4i v, unsigned N, unsigned &bad)
{
    sm_mark<NW>(m, v.x, N, bad); sm_mark<NW>(m, v.y, N, bad); sm_mark<NW>(m, v.z, N, bad); sm_mark<NW>(m, v.w, N, bad);
}

// nclust[row] = number of distinct labels in s[row][0..n), one wavefront per row (row = chain * K + dataset), 4 rows per
// workgroup.  The row starts at any 4-byte boundary (n is arbitrary): up to 3 labels in front of the first 16-byte boundary
// and up to 3 behind the last whole vector are read one per lane, everything between with 16-byte loads, lane-contiguous
// (1 KiB per wave instruction), four in flight per lane.
template <int NW>
__global__ void __launch_bounds__(256) summary_nclust_kernel(const int *__restrict__ s, long long n_rows, long long n, int N,
                                                             int *__restrict__ nclust, int *__restrict__ err)
{
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;                               // (the same in every lane of a wave)
    const int *p = s + row * n;
    unsigned m[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) m[i] = 0u;
    unsigned bad = 0u;
    long long head = (long long)(((16u - (unsigned)((size_t)p & 15u)) & 15u) >> 2);
    if (head > n) head = n;
    if (lane < head) sm_mark<NW>(m, p[lane], (unsigned)N, bad);
    const long long nvec = (n - head) >> 2;
    const sm_v4i *pv = (const sm_v4i *)(p + head);
    long long i = lane;
    for (; i + 192 < nvec; i += 256) {
        const sm_v4i a = pv[i], b = pv[i + 64], c = pv[i + 128], d = pv[i + 192];
        sm_mark4<NW>(m, a, (unsigned)N, bad); sm_mark4<NW>(m, b, (unsigned)N, bad);
        sm_mark4<NW>(m, c, (unsigned)N, bad); sm_mark4<NW>(m, d, (unsigned)N, bad);
    }
    for (; i < nvec; i += 64) sm_mark4<NW>(m, pv[i], (unsigned)N, bad);
    const long long done = head + 4 * nvec;                  // n - done <= 3
    if (done + lane < n) sm_mark<NW>(m, p[done + lane], (unsigned)N, bad);
    // wave-wide OR (butterfly over the 64 lanes), then the population count
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int w = 0; w < NW; ++w) m[w] |= (unsigned)__shfl_xor((int)m[w], off);
        bad |= (unsigned)__shfl_xor((int)bad, off);
    }
    int count = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) count += __popc(m[w]);
    if (lane == 0) {
        nclust[row] = count;
        if (bad) *err = 1;
    }
}

// For the t-th retained value x of a chain: d = x - mean; mean = mean + d / t; m2 = m2 + d * (x - mean) -- three lines of
// separate IEEE double operations, one lane per (chain, scalar): scalar j < K is M[chain][j], the others Phi[chain][j - K].
__global__ void __launch_bounds__(256) summary_welford_kernel(SummaryArgs a, double t)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const int per = a.K + a.npairs;
    if (idx >= (long long)a.C * per) return;
    const long long c = idx / per;
    const int j = (int)(idx - c * per);
    double x, *mean, *m2;
    if (j < a.K) {
        x = a.M[c * a.K + j]; mean = a.M_mean + c * a.K + j; m2 = a.M_m2 + c * a.K + j;
    } else {
        x = a.Phi[c * a.phi_stride + (j - a.K)]; mean = a.Phi_mean + c * a.npairs + (j - a.K); m2 = a.Phi_m2 + c * a.npairs + (j - a.K);
    }
    const double d = x - *mean;
    const double mu = *mean + d / t;
    *mean = mu;
    *m2 = *m2 + d * (x - mu);
}

// dst[j] = ((0.0 + src[0][j]) + src[1][j]) + ... + src[C - 1][j]: the chains are staged through LDS by the whole workgroup
// (coalesced), lane j adds its column in chain order.  stride <= 28 (K <= 8): at least 73 chains per stage.
#define SM_STAGE 2048
__device__ void sm_ordered_sums(const double *__restrict__ src, int C, int stride, int ncols, double *__restrict__ dst, double *stage)
{
    const int chunk = SM_STAGE / stride;
    double acc = 0.0;
    for (long long c0 = 0; c0 < C; c0 += chunk) {
        const int nc = (C - c0 < chunk) ? (int)(C - c0) : chunk;
        for (int i = threadIdx.x; i < nc * stride; i += 256) stage[i] = src[c0 * stride + i];
        __syncthreads();
        if ((int)threadIdx.x < ncols)
            for (int c = 0; c < nc; ++c) acc = acc + stage[c * stride + threadIdx.x];
        __syncthreads();
    }
    if ((int)threadIdx.x < ncols) dst[threadIdx.x] = acc;
}

// Workgroup 0: the cluster counts of this add into the histogram (an LDS histogram first: K (N + 1) <= 2048 bins), the
// per-chain sums of m and m^2, and the trace's sum over chains; workgroups 1 and 2 (launched only while the trace has rows
// left): the trace sums of M and Phi.
__global__ void __launch_bounds__(256) summary_pool_kernel(SummaryArgs a)
{
    __shared__ int h[PMDI_KMAX_I * 256];
    __shared__ double stage[SM_STAGE];
    if (blockIdx.x == 1) { sm_ordered_sums(a.M, a.C, a.K, a.K, a.tr_M, stage); return; }
    if (blockIdx.x == 2) { if (a.npairs > 0) sm_ordered_sums(a.Phi, a.C, a.phi_stride, a.npairs, a.tr_Phi, stage); return; }
    const int tid = threadIdx.x;
    for (int i = tid; i < a.K * 256; i += 256) h[i] = 0;
    __syncthreads();
    const long long rows = (long long)a.C * a.K;
    for (long long i = tid; i < rows; i += 256) {
        const int m = a.nclust[i];                            // 1 .. N (<= 255)
        atomicAdd(&h[(int)(i % a.K) * 256 + m], 1);
        a.nclust_sum[i] += m;
        a.nclust_sumsq[i] += (long long)m * m;
    }
    __syncthreads();
    const int bins = a.N + 1;
    for (int j = tid; j < a.K * bins; j += 256) a.hist[j] += h[(j / bins) * 256 + (j % bins)];
    if (a.tr_nclust && tid < a.K) {
        long long tot = 0;
        for (int m = 0; m < bins; ++m) tot += (long long)m * h[tid * 256 + m];
        a.tr_nclust[tid] = tot;
    }
}

// flag_count[d] += sum over the chains of a slice of flags[chain][d]: lanes along d (coalesced), one integer atomic per lane
__global__ void __launch_bounds__(256) summary_flags_kernel(const unsigned char *__restrict__ flags, int C, long long sumD, int chains_per_block,
                                                            unsigned long long *__restrict__ count)
{
    const long long d = (long long)blockIdx.x * 256 + threadIdx.x;
    if (d >= sumD) return;
    const long long c0 = (long long)blockIdx.y * chains_per_block;
    const long long c1 = (c0 + chains_per_block < C) ? c0 + chains_per_block : C;
    unsigned long long sum = 0;
    for (long long c = c0; c < c1; ++c) sum += flags[c * sumD + d];
    if (sum) atomicAdd(&count[d], sum);
}

}  // namespace

// C K <= INT32_MAX, K <= PMDI_KMAX_I, 2 <= N <= 255 are the caller's to check (pmdi_summary_create).  a.tr_* : this add's
// trace row, or null when the trace is full (or has no rows).
hipError_t pmdi_launch_summary_add(const SummaryArgs &a, long long t, hipStream_t stream)
{
    const long long rows = (long long)a.C * a.K;
    const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    if (a.N <= 32)
        hipLaunchKernelGGL(summary_nclust_kernel<1>, grid, block, 0, stream, a.s, rows, a.n, a.N, a.nclust, a.err);
    else if (a.N <= 64)
        hipLaunchKernelGGL(summary_nclust_kernel<2>, grid, block, 0, stream, a.s, rows, a.n, a.N, a.nclust, a.err);
    else
        hipLaunchKernelGGL(summary_nclust_kernel<8>, grid, block, 0, stream, a.s, rows, a.n, a.N, a.nclust, a.err);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const long long scalars = (long long)a.C * (a.K + a.npairs);
    hipLaunchKernelGGL(summary_welford_kernel, dim3((unsigned)((scalars + 255) / 256)), block, 0, stream, a, (double)t);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(summary_pool_kernel, dim3(a.tr_M ? 3u : 1u), block, 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (a.flags && a.sumD > 0) {
        long long cpb = 64;                                  // chains per workgroup: grid.y <= 65535
        while ((a.C + cpb - 1) / cpb > 65535) cpb *= 2;
        hipLaunchKernelGGL(summary_flags_kernel, dim3((unsigned)((a.sumD + 255) / 256), (unsigned)((a.C + cpb - 1) / cpb)), block, 0, stream,
                           a.flags, a.C, a.sumD, (int)cpb, (unsigned long long *)a.flag_count);
        e = hipGetLastError();
    }
    return e;
}
