// pmdi_mixing.hip -- the streaming mixing accumulator (include/pmdi_hip.h, pmdi_mixing_*): the reference's clustering
// autocorrelation (src/output_analysis/acf_plots.jl:41-59, clustrand: the mean adjusted Rand index between a chain's
// allocations `lag` retained rows apart) and what an effective sample size of M, Phi and the cluster counts needs, taken from
// every retained iteration of every chain on the device.  One add is three launches on the accumulator's stream:
//   mixing_marginal_kernel     one wavefront per (chain, dataset) row: the int32 labels once, as bytes into the ring slot of this
//                              add; the label histogram, P = sum_a h_a (h_a - 1) / 2 and the number of occupied labels
//   mixing_contingency_kernel  the hot path.  One workgroup per row: this add's label bytes staged in LDS, one wavefront per lag;
//                              the contingency table n_ab = sum_i [s_i = a][s'_i = b] of the row against the lagged slot is a
//                              product of one-hot int8 matrices with the observations as the inner dimension
//                              (v_mfma_i32_32x32x32_i8) and lives in the accumulators only: A = sum_ab n_ab (n_ab - 1) / 2
//   mixing_finish_kernel       one lane per (chain, dataset, lag): the pair count and the adjusted Rand index of this add;
//                              one lane per (chain, scalar): the lagged products of M, Phi and the cluster counts
// Every word of the state is owned by one lane of a launch and the launches are ordered on one stream, so the state is
// bit-defined by the order of the adds.
#include <hip/hip_runtime.h>

#include "pmdi_internal.h"
#include "pmdi_onehot.h"            // the fragment types, MX_PAD, mx_wave_sync, mx_wave_sum, mx_onehot

#pragma clang fp contract(off)      // the sums are defined with separate multiplies and adds (the build passes -ffp-contract=off too)

namespace {

// Row `row` = chain * K + dataset of s [rows][n] into ring bytes out [rows][np] (np = n rounded up to 32; the bytes behind n
// are MX_PAD), one wavefront per row, 4 rows per workgroup; a lane packs four consecutive labels into one aligned dword.  The
// histogram of the row is built in the wave's own 256 LDS bins.
__global__ void __launch_bounds__(256) mixing_marginal_kernel(const int *__restrict__ s, long long n_rows, long long n, int np, int N,
                                                              unsigned char *__restrict__ out, long long *__restrict__ P,
                                                              double *__restrict__ nclust, int *__restrict__ err)
{
    __shared__ int hist[4][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row = (long long)blockIdx.x * 4 + wave;
    if (row >= n_rows) return;                               // (the same in every lane of a wave; no workgroup barrier below)
    int *h = hist[wave];
    for (int i = lane; i < 256; i += 64) h[i] = 0;
    mx_wave_sync();
    const int *p = s + row * n;
    unsigned *o = (unsigned *)(out + row * np);
    unsigned bad = 0u;
    const int nd = np >> 2;
#pragma unroll 4
    for (int j = lane; j < nd; j += 64) {
        unsigned u[4], w = 0u;
#pragma unroll
        for (int b = 0; b < 4; ++b) {                        // every address is clamped into the row and the guard selects
            const long long i = 4ll * j + b;                 // afterwards: no load sits under a branch
            u[b] = (unsigned)p[i < n ? i : n - 1];           // a negative label is a large one
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const bool in_row = 4ll * j + b < n, ok = in_row && u[b] < (unsigned)N;
            if (ok) atomicAdd(&h[u[b]], 1);
            bad |= (in_row && !ok) ? 1u : 0u;
            w |= (ok ? u[b] : MX_PAD) << (8 * b);
        }
        o[j] = w;
    }
    mx_wave_sync();
    unsigned long long pairs = 0ull, occupied = 0ull;
    for (int a = lane; a < N; a += 64) {
        const unsigned long long c = (unsigned long long)(unsigned)h[a];      // <= 65535
        pairs += c * (c - 1ull) / 2ull;                      // (c = 0: the product is 0 whatever c - 1 wrapped to)
        occupied += c ? 1ull : 0ull;
    }
    pairs = mx_wave_sum(pairs);
    occupied = mx_wave_sum(occupied);
    bad |= (unsigned)__shfl_xor((int)bad, 32); bad |= (unsigned)__shfl_xor((int)bad, 16); bad |= (unsigned)__shfl_xor((int)bad, 8);
    bad |= (unsigned)__shfl_xor((int)bad, 4); bad |= (unsigned)__shfl_xor((int)bad, 2); bad |= (unsigned)__shfl_xor((int)bad, 1);
    if (lane == 0) {
        P[row] = (long long)pairs;
        nclust[row] = (double)(long long)occupied;
        if (bad) *err = 1;
    }
}

#define MX_CHUNK 1024   // lagged label bytes a wave stages per round: 16 per lane

// A[row][lag - 1] = sum_ab n_ab (n_ab - 1) / 2, n_ab = observations with label a in the row's current slot and label b in the
// slot `lag` adds back, lag = 1..nl.  Workgroup = row; its current bytes [np] are staged once; wave w takes the lags w + 1,
// w + 5, ... and walks the lagged row in rounds of MX_CHUNK bytes through its own staging buffer.  One MFMA covers 32
// observations x (32 x 32) labels: lane (r = lane & 31, h = lane >> 5) holds [s_i == label r] for the 16 observations
// i0 + 16 h .. + 15 as the A fragment and [s'_i == label r] as the B fragment; the hardware pairs byte j of half h on both sides,
// so the sum over the inner dimension runs over the same observation.  NT = 32-label tiles per side of one pass (1: N <= 32,
// 2: N <= 64); GENERIC: passes over the ceil(N / 64)^2 pairs of 64-label blocks.  Only the sum over the table is wanted, so the
// C/D layout (col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 h) does not enter.  After the one workgroup barrier behind the
// staging of the current bytes the waves run apart: a wave's staging buffer is its own and needs wave-level ordering only.
template <int NT, bool GENERIC>
__global__ void __launch_bounds__(256) mixing_contingency_kernel(const unsigned char *__restrict__ ring, long long slot_stride, int np, int N,
                                                                 int cur_slot, int n_slots, int nl, int L, long long *__restrict__ A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char mx_lds[];
    mx_v4u *cur = (mx_v4u *)mx_lds;                          // [np / 16]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    mx_v4u *stage = (mx_v4u *)(mx_lds + np) + wave * (MX_CHUNK / 16);      // [64], this wave's
    const int r = lane & 31, h = lane >> 5;
    const long long row = blockIdx.x;
    {
        const mx_v4u *src = (const mx_v4u *)(ring + (long long)cur_slot * slot_stride + row * np);
        for (int i = tid; i < (np >> 4); i += 256) cur[i] = src[i];
    }
    __syncthreads();
    const int nblk = GENERIC ? (N + 63) >> 6 : 1;
    for (int lag = wave + 1; lag <= nl; lag += 4) {
        const int slot = (cur_slot + n_slots - lag) % n_slots;
        const mx_v4u *lagp = (const mx_v4u *)(ring + (long long)slot * slot_stride + row * np);
        unsigned long long total = 0ull;
        for (int ba = 0; ba < nblk; ++ba)
            for (int bb = 0; bb < nblk; ++bb) {
                unsigned rep_a[NT], rep_b[NT], one_a[NT], one_b[NT];
#pragma unroll
                for (int i = 0; i < NT; ++i) {
                    const unsigned la = (unsigned)(64 * ba + 32 * i + r), lb = (unsigned)(64 * bb + 32 * i + r);
                    rep_a[i] = la * 0x01010101u; one_a[i] = la < (unsigned)N ? 0x01010101u : 0u;
                    rep_b[i] = lb * 0x01010101u; one_b[i] = lb < (unsigned)N ? 0x01010101u : 0u;
                }
                mx_v16i acc[NT][NT];
#pragma unroll
                for (int i = 0; i < NT; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j)
#pragma unroll
                        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0;
                for (int c0 = 0; c0 < np; c0 += MX_CHUNK) {
                    const int left = np - c0;                // a multiple of 32
                    mx_v4u v = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
                    if (16 * lane < left) v = lagp[(c0 >> 4) + lane];
                    mx_wave_sync();                          // the steps of the last round have read the buffer
                    stage[lane] = v;
                    mx_wave_sync();
                    const int steps = left < MX_CHUNK ? left >> 5 : MX_CHUNK / 32;
                    for (int st = 0; st < steps; ++st) {
                        const mx_v4u a16 = cur[(c0 >> 4) + 2 * st + h], b16 = stage[2 * st + h];
                        mx_v4i fa[NT], fb[NT];
#pragma unroll
                        for (int i = 0; i < NT; ++i) { fa[i] = mx_onehot(a16, rep_a[i], one_a[i]); fb[i] = mx_onehot(b16, rep_b[i], one_b[i]); }
#pragma unroll
                        for (int i = 0; i < NT; ++i)
#pragma unroll
                            for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[i], fb[j], acc[i][j], 0, 0, 0);
                    }
                }
#pragma unroll
                for (int i = 0; i < NT; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j)
#pragma unroll
                        for (int e = 0; e < 16; ++e) {
                            const unsigned c = (unsigned)acc[i][j][e];       // <= 65535: c (c - 1) / 2 < 2^31
                            total += (unsigned long long)((c * (c - 1u)) >> 1);
                        }
            }
        total = mx_wave_sum(total);
        if (lane == 0) A[row * L + (lag - 1)] = (long long)total;
    }
}

// Blocks 0 .. blocks_pairs - 1: one lane per (chain, dataset, lag) -- the agreeing pairs and the adjusted Rand index of this
// add against the sample `lag` adds back.  The other blocks: one lane per (chain, scalar j): j < K is M[chain][j], j < K + npairs
// Phi[chain][j - K], the others the cluster counts of this add.  With x1 the chain's first value, y = x - x1.
__global__ void __launch_bounds__(256) mixing_finish_kernel(MixingArgs a, long long t, int nl, int cur_slot, unsigned blocks_pairs)
{
    const int L = a.L, n_slots = a.L + 1;
    const long long rows = (long long)a.C * a.K;
    if (blockIdx.x < blocks_pairs) {
        const long long total = rows * nl;
        for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)blocks_pairs * 256) {
            const long long row = idx / nl;
            const int lag = (int)(idx - row * nl) + 1;
            const int slot = (cur_slot + n_slots - lag) % n_slots;
            const long long Ai = a.A[row * L + (lag - 1)], Pi = a.P_ring[cur_slot * rows + row], Qi = a.P_ring[slot * rows + row];
            const long long T2i = a.n * (a.n - 1) / 2;
            a.rand_num[row * L + (lag - 1)] += T2i + 2 * Ai - Pi - Qi;
            double ari = 1.0;
            if (T2i != 0) {
                const double e = (double)Pi * (double)Qi / (double)T2i;
                const double m = ((double)Pi + (double)Qi) / 2.0;
                const double den = m - e;
                ari = (den == 0.0) ? 1.0 : ((double)Ai - e) / den;
            }
            a.ari_sum[row * L + (lag - 1)] = a.ari_sum[row * L + (lag - 1)] + ari;
        }
        return;
    }
    const long long total = (long long)a.C * a.J, stride = (long long)(gridDim.x - blocks_pairs) * 256;
    for (long long idx = (long long)(blockIdx.x - blocks_pairs) * 256 + threadIdx.x; idx < total; idx += stride) {
        const long long c = idx / a.J;
        const int j = (int)(idx - c * a.J);
        double x;
        if (j < a.K) x = a.M[c * a.K + j];
        else if (j < a.K + a.npairs) x = a.Phi[c * a.phi_stride + (j - a.K)];
        else x = a.nclust[c * a.K + (j - a.K - a.npairs)];
        if (t == 1) a.first[idx] = x;
        const double y = x - a.first[idx];
        a.y_ring[cur_slot * total + idx] = y;
        a.sum_y[idx] = a.sum_y[idx] + y;
        double *prod = a.prod + idx * (L + 1);
        for (int lag = 0; lag <= nl; ++lag) {
            const double z = a.y_ring[((cur_slot + n_slots - lag) % n_slots) * total + idx];
            const double p = y * z;
            prod[lag] = prod[lag] + p;
        }
        if (t <= L) a.head[idx * L + (t - 1)] = y;
        double *tail = a.tail + idx * L;                     // y_{t - L + 1} .. y_t, zero in front of y_1
        for (int i = 0; i < L; ++i) {
            const int back = L - 1 - i;                      // tail[i] = y_{t - back}
            tail[i] = back < t ? a.y_ring[((cur_slot + n_slots - back) % n_slots) * total + idx] : 0.0;
        }
    }
}

template <int NT, bool GENERIC>
hipError_t launch_contingency(const MixingArgs &a, int cur_slot, int nl, hipStream_t stream)
{
    const size_t lds = (size_t)a.np + 4 * MX_CHUNK;
    auto fn = mixing_contingency_kernel<NT, GENERIC>;
    if (lds > 65536) {                                       // (beyond the default limit of dynamic LDS: n > 61 440 only)
        hipError_t e = hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const long long rows = (long long)a.C * a.K;
    hipLaunchKernelGGL(fn, dim3((unsigned)rows), dim3(256), lds, stream, (const unsigned char *)a.ring, rows * a.np, a.np, a.N, cur_slot,
                       a.L + 1, nl, a.L, a.A);
    return hipGetLastError();
}

}  // namespace

// C K <= INT32_MAX, K <= PMDI_KMAX_I, 2 <= N <= 255, 1 <= n <= 65535, 1 <= L <= 1024 are the caller's to check
// (pmdi_mixing_create).  t = 1, 2, ...: the number of this add; its sample goes to ring slot t mod (L + 1).
hipError_t pmdi_launch_mixing_add(const MixingArgs &a, long long t, hipStream_t stream)
{
    const long long rows = (long long)a.C * a.K;
    const int n_slots = a.L + 1, cur_slot = (int)(t % n_slots);
    const int nl = (int)(t - 1 < a.L ? t - 1 : a.L);
    hipLaunchKernelGGL(mixing_marginal_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, a.s, rows, a.n, a.np, a.N,
                       a.ring + (size_t)cur_slot * rows * a.np, a.P_ring + (size_t)cur_slot * rows, a.nclust, a.err);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (nl > 0) {
        e = a.N <= 32 ? launch_contingency<1, false>(a, cur_slot, nl, stream)
          : a.N <= 64 ? launch_contingency<2, false>(a, cur_slot, nl, stream)
                      : launch_contingency<2, true>(a, cur_slot, nl, stream);
        if (e != hipSuccess) return e;
    }
    const long long pair_lanes = rows * nl, scalar_lanes = (long long)a.C * a.J;
    long long bp = (pair_lanes + 255) / 256, bs = (scalar_lanes + 255) / 256;
    if (bp > (1 << 20)) bp = 1 << 20;                        // (the lanes stride over what is left)
    if (bs > (1 << 20)) bs = 1 << 20;
    hipLaunchKernelGGL(mixing_finish_kernel, dim3((unsigned)(bp + bs)), dim3(256), 0, stream, a, t, nl, cur_slot, (unsigned)bp);
    return hipGetLastError();
}
