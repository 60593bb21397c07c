// pmdi_psm_blocksum.hip -- block sums of the posterior-similarity matrices over a grouping of the observations
// (include/pmdi_hip.h, pmdi_psm_blocksum_device): out[m][g][h] = sum_{i in g} sum_{j in h} w^m_ij, the diagonal counted as D.
// With the pixel bins of a dendrogram's leaf order as groups this is the consensus map binned to pixels, with cluster labels
// the cluster x cluster similarity table.  Integer loads and integer sums only: exact in any order.
//
// Two kernels behind one memset of out[0 .. K).
//   psm_blocksum_kernel: ONE WORKGROUP PER (CHUNK, DATASET).  A chunk is at most 32 rows of ONE group g (pmdi_psm_blocksum_plan.h).
//     The workgroup streams its rows counts[k][i][0 .. i) -- the strict lower triangle, nothing else -- as aligned 16-byte loads,
//     reads the four column labels beside them as one aligned 8-byte load (16-bit labels, in the copy shifted to the row's
//     alignment), and adds every w_ij into the LDS bin of group[j] with a 64-bit LDS atomic (ds_add_u64; zero w skipped).  The
//     bins are then L[g][h] = sum_{i in chunk} sum_{j < i, j in h} w_ij for all h: the workgroup adds them into row g of out[k],
//     with plain stores when it is the group's only chunk and with 64-bit integer global atomics when several workgroups feed
//     the group.
//     Up to 128 groups the bins are kept 32 times, one copy per lane residue, and summed at the end: with a handful of labels
//     every lane of a wave would otherwise hit the same few bins and the atomics would serialise.
//   psm_blocksum_finish_kernel: in place, one workgroup per pair of 32 x 32 tiles (bi >= bj) of the G x G tables:
//     out[k][g][h] = L[g][h] + L[h][g] + (g == h ? S |g| : 0), and the Overall table as the sum over k (it is linear in L).
//     Both tiles of a pair are read by this workgroup alone, completely, before it writes either.
//
// Not built: the partial slab T[k][chunk][0 .. G) with a second pass that sums the slab rows of every group.  It needs
// 8 K G (n / 32 + G) bytes of scratch, and the sum over the chunks of one group is serial in the second pass: a labelling with
// one dominant cluster has hundreds of chunks in one group and a handful of lanes adding them up.  Here the pixel regime (every
// group one chunk) makes no atomic at all, and the label regime makes G of them per workgroup, after the workgroup's own sums.
#include <hip/hip_runtime.h>

#include "pmdi_internal.h"
#include "pmdi_psm_device.h"
#include "pmdi_psm_blocksum_plan.h"

namespace {

struct alignas(16) PsmCount4 {
    unsigned v[4];
};
struct alignas(8) PsmLabel4 {
    unsigned short v[4];
};

// grid: x = chunk, y = dataset.  counts may sit at any 4-byte aligned address (a view into a larger tensor): the 16-byte loads are
// aligned on the address itself, and what lies before the first and after the last aligned group of a row is read singly.
template <bool PRIV>
__global__ void __launch_bounds__(256) psm_blocksum_kernel(const int *__restrict__ counts, long long n, int G,
                                                           const unsigned short *__restrict__ g16, long long npad,
                                                           const int *__restrict__ perm, const int *__restrict__ chunk_at,
                                                           const int *__restrict__ chunk_info, unsigned long long *__restrict__ out)
{
    constexpr int NBINS = PRIV ? PSM_BLOCKSUM_GPRIV * 32 : PSM_BLOCKSUM_GMAX_I;
    __shared__ unsigned long long bins[NBINS];
    const int tid = threadIdx.x;
    const int c = blockIdx.x, k = blockIdx.y;
    const int nb = PRIV ? G * 32 : G;
    for (int b = tid; b < nb; b += 256) bins[b] = 0;
    __syncthreads();

    const unsigned long long mis = ((unsigned long long)counts >> 2) & 3ull;      // elements past a 16-byte boundary
    const unsigned *base = (const unsigned *)counts - mis;                            // 16-byte aligned; never read below counts
    const int copy = tid & 31;
    const int r_lo = chunk_at[c], r_hi = chunk_at[c + 1];
    for (int r = r_lo; r < r_hi; ++r) {
        const unsigned long long i = (unsigned long long)perm[r];                    // workgroup-uniform
        const unsigned long long e0 = mis + ((unsigned long long)k * n + i) * n, e1 = e0 + i;     // the row's elements of `base`
        const unsigned long long a0 = (e0 + 3) & ~3ull, a1 = e1 & ~3ull;             // its aligned groups of four: [a0, a1)
        const unsigned long long head_end = a0 < e1 ? a0 : e1;
        const unsigned long long tail_at = a1 > head_end ? a1 : head_end;
        if (tid < (int)(head_end - e0)) {                                            // at most 3 elements
            const unsigned w = base[e0 + tid];
            const unsigned g = g16[tid];
            if (w) atomicAdd(&bins[PRIV ? g * 32 + copy : g], (unsigned long long)w);
        }
        if (tid >= 64 && tid - 64 < (int)(e1 - tail_at)) {                           // at most 3 elements
            const unsigned long long e = tail_at + (unsigned)(tid - 64);
            const unsigned w = base[e];
            const unsigned g = g16[e - e0];
            if (w) atomicAdd(&bins[PRIV ? g * 32 + copy : g], (unsigned long long)w);
        }
        if (a0 < a1) {
            const long long nv = (long long)((a1 - a0) >> 2);
            const PsmCount4 *w4p = (const PsmCount4 *)(base + a0);
            const PsmLabel4 *g4p = (const PsmLabel4 *)(g16 + (a0 - e0) * npad);      // the copy shifted by the row's offset
#pragma unroll 2
            for (long long v = tid; v < nv; v += 256) {
                const PsmCount4 w4 = w4p[v];
                const PsmLabel4 g4 = g4p[v];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (w4.v[u]) atomicAdd(&bins[PRIV ? (unsigned)g4.v[u] * 32 + copy : (unsigned)g4.v[u]], (unsigned long long)w4.v[u]);
            }
        }
    }
    __syncthreads();

    const int info = chunk_info[c];
    unsigned long long *row = out + ((size_t)k * G + (size_t)(info >> 1)) * G;
    for (int h = tid; h < G; h += 256) {
        unsigned long long t = 0;
        if (PRIV) {
            for (int q = 0; q < 32; ++q) t += bins[h * 32 + ((q + h) & 31)];      // rotated: the lanes of a wave on distinct banks
        } else {
            t = bins[h];
        }
        if (info & 1) {
            if (t) atomicAdd(&row[h], t);                                            // several chunks feed this group (out was zeroed)
        } else {
            row[h] = t;
        }
    }
}

// grid: tile pairs of the G x G tables in 32 x 32 tiles.  Thread (rg = tid >> 5, lane = tid & 31) holds rows rg + 8 e, e < 4,
// column `lane` of both tiles of its pair.
__global__ void __launch_bounds__(256) psm_blocksum_finish_kernel(unsigned long long *out, int K, int G, const int *__restrict__ gsize,
                                                                  long long S)
{
    __shared__ unsigned long long t[32][33];
    const int tid = threadIdx.x, lane = tid & 31, rg = tid >> 5;
    int bi, bj;
    psm_tile_pair(blockIdx.x, bi, bj);
    const int i0 = bi * 32, j0 = bj * 32;
    const size_t GG = (size_t)G * G;
    unsigned long long at[4], bt[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) at[e] = bt[e] = 0;
    const int M = K + (K > 1 ? 1 : 0);
    for (int m = 0; m < M; ++m) {
        unsigned long long a[4], b[4];
        unsigned long long *o = out + (size_t)m * GG;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int rr = rg + 8 * e;
            if (m < K) {
                a[e] = (i0 + rr < G && j0 + lane < G) ? o[(size_t)(i0 + rr) * G + j0 + lane] : 0ull;      // L[g][h], tile (bi, bj)
                b[e] = (j0 + rr < G && i0 + lane < G) ? o[(size_t)(j0 + rr) * G + i0 + lane] : 0ull;      // L[h'][g'], tile (bj, bi)
                at[e] += a[e];
                bt[e] += b[e];
            } else {
                a[e] = at[e];
                b[e] = bt[e];
            }
        }
        const unsigned long long D = (unsigned long long)S * (unsigned long long)(m < K ? 1 : K);
        __syncthreads();                                   // the last round's reads of t are done
#pragma unroll
        for (int e = 0; e < 4; ++e) t[rg + 8 * e][lane] = b[e];
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int g = i0 + rg + 8 * e, h = j0 + lane;
            if (g < G && h < G) o[(size_t)g * G + h] = a[e] + t[lane][rg + 8 * e] + (g == h ? D * (unsigned long long)gsize[g] : 0ull);
        }
        if (bi != bj) {                                    // workgroup-uniform
            __syncthreads();
#pragma unroll
            for (int e = 0; e < 4; ++e) t[rg + 8 * e][lane] = a[e];
            __syncthreads();
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int h = j0 + rg + 8 * e, g = i0 + lane;
                if (h < G && g < G) o[(size_t)h * G + g] = b[e] + t[lane][rg + 8 * e];
            }
        }
    }
}

}  // namespace

// The tables of PsmBlocksumPlan on the device; out [K + (K > 1)][G][G], every element written.  1 <= n <= 65535,
// 1 <= G <= PSM_BLOCKSUM_GMAX_I, 1 <= K and 1 <= nchunks <= n are the caller's to check.
hipError_t pmdi_launch_psm_blocksum(const int *counts, long long S, int K, long long n, int G, const unsigned short *g16, long long npad,
                                    const int *perm, const int *chunk_at, const int *chunk_info, int nchunks, const int *gsize,
                                    unsigned long long *out, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(out, 0, (size_t)K * G * G * sizeof(unsigned long long), stream);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)nchunks, (unsigned)K);
    if (G <= PSM_BLOCKSUM_GPRIV)
        hipLaunchKernelGGL(psm_blocksum_kernel<true>, grid, dim3(256), 0, stream, counts, n, G, g16, npad, perm, chunk_at, chunk_info, out);
    else
        hipLaunchKernelGGL(psm_blocksum_kernel<false>, grid, dim3(256), 0, stream, counts, n, G, g16, npad, perm, chunk_at, chunk_info, out);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(psm_blocksum_finish_kernel, dim3(psm_tile_pairs(G, 32)), dim3(256), 0, stream, out, K, G, gsize, S);
    return hipGetLastError();
}
