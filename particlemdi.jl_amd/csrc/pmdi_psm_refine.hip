// pmdi_psm_refine.hip -- coordinate descent of Binder's loss from given start clusterings (include/pmdi_hip.h,
// pmdi_psm_refine_device).  One sweep visits i = 0 .. n - 1 in index order; i is taken out of its group, every live group g
// is offered with gain(g) = 2 A_i(g) - D |g|, A_i(g) = sum_{j in g, j != i} w_ij, a new singleton with gain 0, and the first
// option with the largest gain in the order (i's own group, the other groups by ascending slot, the new singleton) wins.
// The gains are integers, so the descent is the same on every run and on every machine.
//
// Two kernels.
//   psm_refine_build_kernel: the symmetric n x n uint32 work matrix of w for the chosen matrix, from the lower triangle of
//     the counts (64 x 64 tiles, the mirror image written through LDS so that both halves are coalesced); diagonal 0, so
//     that j != i needs no test later; for the Overall matrix the sum over the K datasets is paid once, not once per visit.
//   psm_refine_kernel: ONE PERSISTENT WORKGROUP PER START (16 waves).  A visit is two phases and two barriers: all waves
//     read row i of the work matrix (coalesced) and the labels and add w_ij into the bin of label[j] with LDS atomics (zero w
//     skipped); then wave 0 alone scans the used slots (reading and clearing the bins in one pass), reduces (gain, slot)
//     with shuffles, decides, and updates the label and the group sizes.  The labels live in the output array (global, read
//     and written by this workgroup only); bins and sizes of all PMDI_REFINE_GMAX slots live in LDS.  Nothing waits on
//     another workgroup: the starts only share the work matrix through L2.
//
// Not built: an n x G table of A_j(g) per start updated only when an observation moves (a visit would cost G reads instead of
// n, but the table is n G 8 bytes per start: 0.3 GB at n = 10 000 for ONE start with G = 4096); wave-private bins reduced at
// the end of a visit (G x 16 x 8 bytes of LDS, and lanes of one wave that hit one bin serialise in either form).
#include <hip/hip_runtime.h>

#include "pmdi_internal.h"
#include "pmdi_psm_device.h"

namespace {

#define PSM_REFINE_G PMDI_REFINE_GMAX_I
#define PSM_REFINE_THREADS 1024

__global__ void __launch_bounds__(256) psm_refine_build_kernel(const int *__restrict__ counts, int K, long long n, int which,
                                                               unsigned n_tile_pairs, unsigned *__restrict__ W)
{
    __shared__ unsigned t[64][65];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int k_lo, k_hi;
    psm_k_range(which, K, k_lo, k_hi);
    for (unsigned p = blockIdx.x; p < n_tile_pairs; p += gridDim.x) {
        int bi, bj;
        psm_tile_pair_uniform(p, bi, bj);
        const long long i0 = (long long)bi * 64, j0 = (long long)bj * 64;
        for (int rr = wave; rr < 64; rr += 4) {
            const long long i = i0 + rr, j = j0 + lane;
            unsigned w = 0;
            if (i < n && j < i) w = psm_w<unsigned>(counts, k_lo, k_hi, n, i, j);
            t[rr][lane] = w;
            if (i < n && j <= i) W[(size_t)i * n + j] = w;                      // the lower half and the diagonal (0)
        }
        __syncthreads();
        for (int rr = wave; rr < 64; rr += 4) {
            const long long j = j0 + rr, i = i0 + lane;                         // element (j, i) of the mirror image
            if (i < n && j < i) W[(size_t)j * n + i] = t[lane][rr];
        }
        __syncthreads();
    }
}

// BT = unsigned: the caller guarantees D n < 2^32, so A_i(g) <= D (n - 1) fits; BT = unsigned long long otherwise.
template <typename BT>
__global__ void __launch_bounds__(PSM_REFINE_THREADS) psm_refine_kernel(const unsigned *__restrict__ W, long long n, long long D,
                                                                        const int *__restrict__ start, long long ld, int max_sweeps,
                                                                        int *labels, long long *__restrict__ moves_out,
                                                                        int *__restrict__ sweeps_out, int *__restrict__ flag)
{
    __shared__ BT bins[PSM_REFINE_G];
    __shared__ int gsz[PSM_REFINE_G];
    __shared__ int s_hi, s_bad, s_moved;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long b = blockIdx.x;
    int *lab = labels + (size_t)b * n;
    const int *st = start + (size_t)b * ld;

    for (int g = tid; g < PSM_REFINE_G; g += PSM_REFINE_THREADS) { bins[g] = 0; gsz[g] = 0; }
    if (tid == 0) { s_hi = 0; s_bad = 0; s_moved = 0; }
    __syncthreads();
    {
        int hi_l = 0, bad = 0;
        for (long long j = tid; j < n; j += PSM_REFINE_THREADS) {
            const int v = st[j];
            if ((unsigned)v >= (unsigned)PSM_REFINE_G) bad = 1;
            else { atomicAdd(&gsz[v], 1); hi_l = v + 1 > hi_l ? v + 1 : hi_l; }
            lab[j] = v;
        }
        if (bad) s_bad = 1;
        if (hi_l) atomicMax(&s_hi, hi_l);
    }
    __syncthreads();
    if (s_bad) {                                                   // workgroup-uniform: a start label outside the slot range
        if (tid == 0) { atomicOr(flag, 1); moves_out[b] = 0; sweeps_out[b] = 0; }
        return;
    }

    // wave 0 keeps these, uniform over its lanes
    int hi = s_hi, live = 0;
    if (wave == 0) {
        for (int g = lane; g < hi; g += 64) live += gsz[g] > 0 ? 1 : 0;
        for (int off = 32; off > 0; off >>= 1) live += __shfl_xor(live, off, 64);
    }
    long long moves = 0;
    int sweeps = 0;

    for (int sweep = 0; sweep < max_sweeps; ++sweep) {
        int moved = 0;
        for (long long i = 0; i < n; ++i) {
            const unsigned *row = W + (size_t)i * n;
            for (long long base = tid; base < n; base += 4 * PSM_REFINE_THREADS) {
                unsigned w[4];
                int l[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const long long j = base + (long long)u * PSM_REFINE_THREADS;
                    w[u] = j < n ? row[j] : 0u;
                    l[u] = j < n ? lab[j] : 0;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (w[u]) atomicAdd(&bins[l[u]], (BT)w[u]);
            }
            __syncthreads();
            if (wave == 0) {
                const int cur = lab[i];
                const long long a_cur = (long long)bins[cur];
                const int sz_cur = gsz[cur];
                long long bg = 0;
                int bs = -1;
                for (int g = lane; g < hi; g += 64) {                          // ascending slots: a lane keeps its lowest best
                    const long long a = (long long)bins[g];
                    const int sz = gsz[g];
                    bins[g] = 0;
                    if (g != cur && sz > 0) {
                        const long long gain = 2 * a - D * (long long)sz;
                        if (bs < 0 || gain > bg) { bg = gain; bs = g; }
                    }
                }
                for (int off = 32; off > 0; off >>= 1) {
                    const long long og = __shfl_xor(bg, off, 64);
                    const int os = __shfl_xor(bs, off, 64);
                    if (os >= 0 && (bs < 0 || og > bg || (og == bg && os < bs))) { bg = og; bs = os; }
                }
                const bool alone = sz_cur == 1;
                long long tg = alone ? 0 : 2 * a_cur - D * (long long)(sz_cur - 1);
                int target = cur;
                if (bs >= 0 && bg > tg) { target = bs; tg = bg; }
                if (!alone && live < PSM_REFINE_G && tg < 0) {                 // the new singleton: the lowest free slot
                    int f = PSM_REFINE_G;
                    for (int g = lane; g < PSM_REFINE_G; g += 64)
                        if (gsz[g] == 0) { f = g; break; }
                    for (int off = 32; off > 0; off >>= 1) {
                        const int o = __shfl_xor(f, off, 64);
                        f = o < f ? o : f;
                    }
                    target = f;
                }
                if (target != cur) {
                    const bool fresh = gsz[target] == 0;
                    if (lane == 0) { gsz[cur] = sz_cur - 1; gsz[target] += 1; lab[i] = target; }
                    live += (fresh ? 1 : 0) - (alone ? 1 : 0);
                    hi = target + 1 > hi ? target + 1 : hi;
                    ++moves;
                    moved = 1;
                }
            }
            __syncthreads();
        }
        ++sweeps;
        if (tid == 0) s_moved = moved;
        __syncthreads();
        const int any = s_moved;
        __syncthreads();
        if (!any) break;
    }
    if (tid == 0) { moves_out[b] = moves; sweeps_out[b] = sweeps; }
}

}  // namespace

// The work matrix of both descents (this one and pmdi_psm_refine_vi.hip): W = n x n uint32, every element written.
hipError_t pmdi_launch_psm_refine_build(const int *counts, int K, long long n, int which, unsigned *W, hipStream_t stream)
{
    const unsigned tile_pairs = psm_tile_pairs(n, 64);
    hipLaunchKernelGGL(psm_refine_build_kernel, dim3(tile_pairs < 8192u ? tile_pairs : 8192u), dim3(256), 0, stream, counts, K, n, which,
                       tile_pairs, W);
    return hipGetLastError();
}

// W: n x n uint32 work space.  labels [B][n], moves [B], sweeps [B], flag [1] (zero before the launch) on the device.
// wide: D n >= 2^32.  1 <= n <= 65535, 1 <= B, D <= 2^31 - 1 and max_sweeps >= 1 are the caller's to check.
hipError_t pmdi_launch_psm_refine(const int *counts, int K, long long n, int which, long long D, int wide, unsigned *W, const int *start,
                                  long long B, long long ld, int max_sweeps, int *labels, long long *moves, int *sweeps, int *flag,
                                  hipStream_t stream)
{
    hipError_t e = pmdi_launch_psm_refine_build(counts, K, n, which, W, stream);
    if (e != hipSuccess) return e;
    const long long slab = 1LL << 20;                // starts per launch
    for (long long at = 0; at < B; at += slab) {
        const long long nb = B - at < slab ? B - at : slab;
        if (wide)
            hipLaunchKernelGGL(psm_refine_kernel<unsigned long long>, dim3((unsigned)nb), dim3(PSM_REFINE_THREADS), 0, stream, W, n, D,
                               start + (size_t)at * ld, ld, max_sweeps, labels + (size_t)at * n, moves + at, sweeps + at, flag);
        else
            hipLaunchKernelGGL(psm_refine_kernel<unsigned>, dim3((unsigned)nb), dim3(PSM_REFINE_THREADS), 0, stream, W, n, D,
                               start + (size_t)at * ld, ld, max_sweeps, labels + (size_t)at * n, moves + at, sweeps + at, flag);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
