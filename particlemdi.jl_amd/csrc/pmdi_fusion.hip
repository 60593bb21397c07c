// pmdi_fusion.hip -- the streaming fusion accumulator (include/pmdi_hip.h, pmdi_fusion_*).  A group g is a set of two or more
// datasets, given as a bit mask; observation i is fused across g in sample t when every member of g gives it the same label:
//   fused[g][i]     += sum_t f_g(t, i)
//   counts[g][i][j] += sum_t f_g(t, i) f_g(t, j) [label of i == label of j]        (so counts[g][i][i] = fused[g][i])
// The counting kernels are the bodies of pmdi_psm_device.h with the fused staging rule (PsmStageFused) and grid.y = group:
// the accumulating, lower-tile-triangle kernels of pmdi_psm_acc.hip over "the shared label, or nothing".  Nothing of size
// S G n is ever written to global memory.  Mirror and merge are pmdi_psm_acc.hip's, with K := G.
// Integer compares, int8 products and int32 sums only: exact by construction.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pmdi_internal.h"
#include "pmdi_psm_device.h"

namespace {

// The groups of one launch have at most NM members each (NM = 2, 4, 8: the staging rule's loads are unrolled over NM); `order`
// lists the accumulator's groups by that class, and this launch takes order[first], order[first + 1], ...

// grid: x = tile pair (64-wide tiles), y = group of the class.  Staged values are 16 bits wide: the label, or 0x100 / 0x200 for an
// observation that is not fused (and for the padding) -- with n_labels = 0 every byte is a label and none is free to mean "nothing".
template <int NM>
__global__ void __launch_bounds__(256) fusion_acc_kernel(const unsigned char *__restrict__ samples, long long S, int K, long long n,
                                                         const unsigned char *__restrict__ masks, const unsigned char *__restrict__ order,
                                                         int first, int *__restrict__ counts)
{
    const int g = order[first + blockIdx.y];
    int bi, bj;
    psm_tile_pair(blockIdx.x, bi, bj);
    psm_count_body<true>(PsmStageFused<unsigned short, NM>(masks[g]), samples, S, K, n, g, (long long)bi * 64, (long long)bj * 64, n, n, 0,
                         counts);
}

// grid: x = tile pair (128-wide tiles), y = group of the class.  Labels < 32 NKB: byte 255 / 254 has an all-zero one-hot row, as
// the padding.  4 waves per SIMD asked for, as psm_acc_mfma_kernel does and for its reason.
template <int NKB, int NM>
__global__ void __launch_bounds__(256, 4) fusion_acc_mfma_kernel(const unsigned char *__restrict__ samples, long long S, int K, long long n,
                                                              const unsigned char *__restrict__ masks,
                                                              const unsigned char *__restrict__ order, int first, int *__restrict__ counts)
{
    const int g = order[first + blockIdx.y];
    int bi, bj;
    psm_tile_pair(blockIdx.x, bi, bj);
    psm_count_mfma_body<NKB, true>(PsmStageFused<unsigned char, NM>(masks[g]), samples, S, K, n, g, (long long)bi * 128,
                                   (long long)bj * 128, n, n, 0, counts);
}

// The matrix-free add: fused[g][i] += #{t : i is fused across g}.  grid: x = 256 lanes of W observations, y = FUS_TR samples.  A lane
// reads the labels of its W = 4 consecutive observations (n a multiple of 4 and an aligned batch; W = 1 otherwise) in one dataset
// as one dword, KT datasets per sample (K <= KT; a dataset >= K repeats the last one), no load under a branch.  The members of a
// group agree in a byte iff their OR equals their AND there; a packed byte counter per group counts the samples in which they do
// NOT (at most FUS_TR <= 255 per byte).  Eight groups (four when K > 4) per pass over the labels; one integer atomic per (group, observation, block):
// the sum is exact in any order.
#define FUS_TR 32
template <int KT, bool VEC>
__global__ void __launch_bounds__(256) fusion_obs_kernel(const unsigned char *__restrict__ samples, long long S, int K, long long n,
                                                         const unsigned char *__restrict__ masks, int G, int *__restrict__ fused)
{
    constexpr int W = VEC ? 4 : 1, GP = KT > 4 ? 4 : 8;            // groups per pass: their member selectors stay in scalar registers
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * W;
    const long long t0 = (long long)blockIdx.y * FUS_TR;
    const int nt = (int)(S - t0 < FUS_TR ? S - t0 : FUS_TR);       // workgroup-uniform, >= 1
    if (i >= n) return;
    for (int g0 = 0; g0 < G; g0 += GP) {
        unsigned sel[GP][KT];                                        // workgroup-uniform: all ones where dataset k is a member
#pragma unroll
        for (int j = 0; j < GP; ++j) {
            const unsigned m = g0 + j < G ? masks[g0 + j] : 0u;
#pragma unroll
            for (int k = 0; k < KT; ++k) sel[j][k] = (m >> k) & 1u ? 0xffffffffu : 0u;
        }
        unsigned unfused[GP] = {};
#pragma unroll 4
        for (int tt = 0; tt < FUS_TR; ++tt) {
            const unsigned char *row = samples + (size_t)(t0 + (tt < nt ? tt : nt - 1)) * K * n + i;
            unsigned w[KT];
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                const unsigned char *p = row + (size_t)(k < K ? k : K - 1) * n;
                w[k] = VEC ? *(const unsigned *)p : (unsigned)*p;
            }
            const unsigned live = tt < nt ? 0x01010101u : 0u;
#pragma unroll
            for (int j = 0; j < GP; ++j) {
                unsigned any = 0u, all = 0xffffffffu;
#pragma unroll
                for (int k = 0; k < KT; ++k) { any |= w[k] & sel[j][k]; all &= w[k] | ~sel[j][k]; }
                const unsigned x = any ^ all;                       // a byte is zero iff the members agree in it
                unfused[j] += ((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) >> 7) & live;
            }
        }
#pragma unroll
        for (int j = 0; j < GP; ++j) {
            if (g0 + j >= G) break;
#pragma unroll
            for (int b = 0; b < W; ++b) {
                const int c = nt - (int)((unfused[j] >> (8 * b)) & 0xffu);
                if (c) atomicAdd(&fused[(size_t)(g0 + j) * n + i + b], c);
            }
        }
    }
}

// fused[g][i] = counts[g][i][i]: what the matrix mode reports as fused
__global__ void __launch_bounds__(256) fusion_diag_kernel(const int *__restrict__ counts, long long n, int *__restrict__ fused)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) fused[(size_t)blockIdx.y * n + i] = counts[((size_t)blockIdx.y * n + i) * n + i];
}

// a[x] += b[x]: the merge of the matrix-free mode
__global__ void __launch_bounds__(256) fusion_add_kernel(int *__restrict__ a, const int *__restrict__ b, long long count)
{
    const long long x = (long long)blockIdx.x * 256 + threadIdx.x;
    if (x < count) a[x] += b[x];
}

}  // namespace

// n <= 65535, K <= PMDI_KMAX_I and G <= 247 masks of two or more bits below K are the caller's to check (pmdi_fusion_create);
// order = the groups sorted by class (2, 3..4, 5..8 members), n_class[c] of them in class c
hipError_t pmdi_launch_fusion_add(const unsigned char *samples, long long S, int K, long long n, int n_labels, const unsigned char *masks,
                                  const unsigned char *order, const int *n_class, int *counts, hipStream_t stream)
{
    if (S <= 0 || n <= 0) return hipSuccess;
    const int path = n_labels >= 1 && n_labels <= 32 ? 1 : n_labels >= 1 && n_labels <= 64 ? 2 : 0;
    const dim3 block(256);
    int first = 0;
    for (int c = 0; c < 3; first += n_class[c++]) {
        if (n_class[c] <= 0) continue;
        const dim3 grid(psm_tile_pairs(n, path ? 128 : 64), (unsigned)n_class[c]);
#define FUS_LAUNCH(NM)                                                                                                                 \
        if (path == 1) hipLaunchKernelGGL((fusion_acc_mfma_kernel<1, NM>), grid, block, 0, stream, samples, S, K, n, masks, order, first, counts);      \
        else if (path == 2) hipLaunchKernelGGL((fusion_acc_mfma_kernel<2, NM>), grid, block, 0, stream, samples, S, K, n, masks, order, first, counts); \
        else hipLaunchKernelGGL((fusion_acc_kernel<NM>), grid, block, 0, stream, samples, S, K, n, masks, order, first, counts)
        if (c == 0) { FUS_LAUNCH(2); } else if (c == 1) { FUS_LAUNCH(4); } else { FUS_LAUNCH(8); }
#undef FUS_LAUNCH
    }
    return hipGetLastError();
}

// S <= INT32_MAX (pmdi_fusion_add_samples): grid.y fits
hipError_t pmdi_launch_fusion_obs(const unsigned char *samples, long long S, int K, long long n, const unsigned char *masks, int G, int *fused,
                                  hipStream_t stream)
{
    if (S <= 0 || n <= 0 || G <= 0) return hipSuccess;
    const bool vec = n % 4 == 0 && (uintptr_t)samples % 4 == 0;
    const long long lanes = vec ? n / 4 : n;
    const long long per = 65535LL * FUS_TR;                      // samples one launch takes (grid.y <= 65535)
    for (long long at = 0; at < S; at += per) {
        const long long s = S - at < per ? S - at : per;
        const dim3 grid((unsigned)((lanes + 255) / 256), (unsigned)((s + FUS_TR - 1) / FUS_TR)), block(256);
        const unsigned char *smp = samples + (size_t)at * K * n;   // (per K n is a multiple of 4: the alignment holds)
#define FUS_LAUNCH(KT)                                                                                                        \
        if (vec) hipLaunchKernelGGL((fusion_obs_kernel<KT, true>), grid, block, 0, stream, smp, s, K, n, masks, G, fused);    \
        else hipLaunchKernelGGL((fusion_obs_kernel<KT, false>), grid, block, 0, stream, smp, s, K, n, masks, G, fused)
        if (K <= 2) { FUS_LAUNCH(2); } else if (K <= 4) { FUS_LAUNCH(4); } else { FUS_LAUNCH(8); }
#undef FUS_LAUNCH
    }
    return hipGetLastError();
}

hipError_t pmdi_launch_fusion_diag(const int *counts, int G, long long n, int *fused, hipStream_t stream)
{
    if (n <= 0 || G <= 0) return hipSuccess;
    hipLaunchKernelGGL(fusion_diag_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)G), dim3(256), 0, stream, counts, n, fused);
    return hipGetLastError();
}

hipError_t pmdi_launch_fusion_merge_obs(int *a, const int *b, int G, long long n, hipStream_t stream)
{
    if (n <= 0 || G <= 0) return hipSuccess;
    const long long count = (long long)G * n;
    hipLaunchKernelGGL(fusion_add_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, a, b, count);
    return hipGetLastError();
}
