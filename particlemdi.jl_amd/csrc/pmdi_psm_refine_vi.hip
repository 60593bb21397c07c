// pmdi_psm_refine_vi.hip -- coordinate descent of the Wade-Ghahramani VI bound from given start clusterings (include/pmdi_hip.h,
// pmdi_psm_refine_vi_device).  The objective is F(c) = sum_g [ |g| L(|g|) - 2 sum_{j in g} L(own_j + D) ] with the fixed-point
// logarithm L (integer arithmetic only, the same bits on the host, here and in tests/_np_vi_refine.py), so every gain is an exact
// int64 and the descent is the same on every run and on every machine.  Visiting order, ranking of the options and the tie rule
// are those of pmdi_psm_refine.hip; the n x n uint32 work matrix and its build kernel are shared with it.
//
// psm_refine_vi_kernel: ONE PERSISTENT WORKGROUP PER START (16 waves).  own_j = A_j(c_j) of every observation lives in global
// memory (n int64 per start, read and written by this workgroup only; first formed by one pass over the work matrix, a wave per
// row).  A visit of i is three phases:
//   1. all waves read row i, label[j] and own[j] and, for w_ij != 0, add w_ij into A[label[j]] and the change of L(own_j + D)
//      that moving i would cause into R[label[j]] (own_j - w_ij for i's own group, own_j + w_ij for any other), with 64-bit LDS
//      atomics: integer adds, exact in any order;
//   2. wave 0 scans the used slots (reading and clearing A and R in one pass), forms the gains, reduces (gain, slot) with shuffles
//      under the tie rule and decides;
//   3. only when i moved, all waves pass over row i again: own[j] -= w_ij in the old group, own[j] += w_ij in the new one,
//      own[i] = A_i(new).
// Two barriers per visit, a third on a move.  LDS: A 32 KiB, R 32 KiB, sizes 16 KiB, the table 8 KiB.
//
// Not built: L(own_j + D) cached per observation (one L less per non-zero w in phase 1, one more array of n int64 per start to
// keep in step in phase 3); 32-bit A when D n < 2^32 (R needs 64 bits whatever D is); the n x G table of pmdi_psm_refine.hip's
// remarks, for the same reason as there.
#include <hip/hip_runtime.h>

#include "pmdi_fixlog.h"            // L and s L(s)
#include "pmdi_internal.h"

namespace {

#define PSM_VI_G PMDI_REFINE_GMAX_I
#define PSM_VI_THREADS 1024
#define PSM_VI_TABLE PMDI_FIXLOG_TABLE

__device__ const int psm_vi_table[PSM_VI_TABLE] = {
#include "pmdi_vi_log2_table.h"
};

__global__ void __launch_bounds__(PSM_VI_THREADS) psm_refine_vi_kernel(const unsigned *__restrict__ W, long long n, long long D,
                                                                       const int *__restrict__ start, long long ld, int max_sweeps,
                                                                       int *labels, long long *own_all, long long *__restrict__ moves_out,
                                                                       int *__restrict__ sweeps_out, long long *__restrict__ objective_out,
                                                                       int *__restrict__ flag)
{
    __shared__ unsigned long long A[PSM_VI_G];          // A_i(g) of the visit
    __shared__ unsigned long long R[PSM_VI_G];          // sum over j in g of the change of L(own_j + D), two's complement
    __shared__ int gsz[PSM_VI_G];
    __shared__ int T[PSM_VI_TABLE];
    __shared__ unsigned long long s_anew, s_obj;
    __shared__ int s_hi, s_bad, s_moved, s_to;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long b = blockIdx.x;
    int *lab = labels + (size_t)b * n;
    long long *own = own_all + (size_t)b * n;
    const int *st = start + (size_t)b * ld;

    for (int g = tid; g < PSM_VI_G; g += PSM_VI_THREADS) { A[g] = 0; R[g] = 0; gsz[g] = 0; }
    for (int k = tid; k < PSM_VI_TABLE; k += PSM_VI_THREADS) T[k] = psm_vi_table[k];
    if (tid == 0) { s_hi = 0; s_bad = 0; s_moved = 0; s_to = -1; s_anew = 0; s_obj = 0; }
    __syncthreads();
    {
        int hi_l = 0, bad = 0;
        for (long long j = tid; j < n; j += PSM_VI_THREADS) {
            const int v = st[j];
            if ((unsigned)v >= (unsigned)PSM_VI_G) bad = 1;
            else { atomicAdd(&gsz[v], 1); hi_l = v + 1 > hi_l ? v + 1 : hi_l; }
            lab[j] = v;
        }
        if (bad) s_bad = 1;
        if (hi_l) atomicMax(&s_hi, hi_l);
    }
    __syncthreads();
    if (s_bad) {                                                   // workgroup-uniform: a start label outside the slot range
        if (tid == 0) { atomicOr(flag, 1); moves_out[b] = 0; sweeps_out[b] = 0; objective_out[b] = 0; }
        return;
    }

    for (long long j = wave; j < n; j += PSM_VI_THREADS / 64) {    // own_j of the start: a wave per row
        const unsigned *row = W + (size_t)j * n;
        const int lj = lab[j];
        long long s = 0;
        for (long long k = lane; k < n; k += 64) s += lab[k] == lj ? (long long)row[k] : 0;      // w_jj = 0
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        if (lane == 0) own[j] = s;
    }

    // wave 0 keeps these, uniform over its lanes
    int hi = s_hi, live = 0;
    if (wave == 0) {
        for (int g = lane; g < hi; g += 64) live += gsz[g] > 0 ? 1 : 0;
        for (int off = 32; off > 0; off >>= 1) live += __shfl_xor(live, off, 64);
    }
    long long moves = 0;
    int sweeps = 0;
    __syncthreads();

    for (int sweep = 0; sweep < max_sweeps; ++sweep) {
        int moved = 0;
        for (long long i = 0; i < n; ++i) {
            const unsigned *row = W + (size_t)i * n;
            const int cur = lab[i];
            for (long long base = tid; base < n; base += 4 * PSM_VI_THREADS) {
                unsigned w[4];
                int l[4];
                long long o[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const long long j = base + (long long)u * PSM_VI_THREADS;
                    w[u] = j < n ? row[j] : 0u;
                    l[u] = j < n ? lab[j] : 0;
                    o[u] = j < n ? own[j] : 0;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (w[u]) {                                                // own_j >= w_ij inside i's group: the argument stays >= D
                        const unsigned long long od = (unsigned long long)(o[u] + D);
                        const unsigned long long om = l[u] == cur ? od - w[u] : od + w[u];      // after i has moved
                        atomicAdd(&A[l[u]], (unsigned long long)w[u]);
                        atomicAdd(&R[l[u]], (unsigned long long)(pmdi_fixlog_L(om, T) - pmdi_fixlog_L(od, T)));
                    }
            }
            __syncthreads();
            if (wave == 0) {
                const long long a_cur = (long long)A[cur];
                const int sz_cur = gsz[cur];
                const bool alone = sz_cur == 1;
                // what leaving the current group gains, the same for every destination
                const long long leave = pmdi_fixlog_sL(sz_cur, T) - pmdi_fixlog_sL(sz_cur - 1, T) + 2 * (long long)R[cur]
                                        - 2 * pmdi_fixlog_L((unsigned long long)(a_cur + D), T);
                long long bg = 0, ba = 0;
                int bs = -1;
                for (int g = lane; g < hi; g += 64) {                          // ascending slots: a lane keeps its lowest best
                    const long long a = (long long)A[g], r = (long long)R[g];
                    const int sz = gsz[g];
                    A[g] = 0; R[g] = 0;
                    if (g != cur && sz > 0) {
                        const long long gain = leave - (pmdi_fixlog_sL(sz + 1, T) - pmdi_fixlog_sL(sz, T)) + 2 * r
                                               + 2 * pmdi_fixlog_L((unsigned long long)(a + D), T);
                        if (bs < 0 || gain > bg) { bg = gain; bs = g; ba = a; }
                    }
                }
                for (int off = 32; off > 0; off >>= 1) {
                    const long long og = __shfl_xor(bg, off, 64), oa = __shfl_xor(ba, off, 64);
                    const int os = __shfl_xor(bs, off, 64);
                    if (os >= 0 && (bs < 0 || og > bg || (og == bg && os < bs))) { bg = og; bs = os; ba = oa; }
                }
                long long tg = 0, a_new = a_cur;                               // the current group: gain 0
                int target = cur;
                if (bs >= 0 && bg > tg) { target = bs; tg = bg; a_new = ba; }
                if (!alone && live < PSM_VI_G && leave + 2 * pmdi_fixlog_L((unsigned long long)D, T) > tg) {     // the new singleton: the lowest free slot
                    int f = PSM_VI_G;
                    for (int g = lane; g < PSM_VI_G; g += 64)
                        if (gsz[g] == 0) { f = g; break; }
                    for (int off = 32; off > 0; off >>= 1) {
                        const int o = __shfl_xor(f, off, 64);
                        f = o < f ? o : f;
                    }
                    target = f;
                    a_new = 0;
                }
                if (target != cur) {
                    const bool fresh = gsz[target] == 0;
                    if (lane == 0) {
                        gsz[cur] = sz_cur - 1; gsz[target] += 1; lab[i] = target;
                        s_to = target; s_anew = (unsigned long long)a_new;
                    }
                    live += (fresh ? 1 : 0) - (alone ? 1 : 0);
                    hi = target + 1 > hi ? target + 1 : hi;
                    ++moves;
                    moved = 1;
                } else if (lane == 0) s_to = -1;
            }
            __syncthreads();
            const int to = s_to;                                               // workgroup-uniform; next written after the next barrier
            if (to >= 0) {
                for (long long j = tid; j < n; j += PSM_VI_THREADS) {
                    const unsigned w = row[j];
                    if (w) {                                                   // w_ii = 0: i itself is not touched here
                        const int l = lab[j];
                        if (l == cur) own[j] -= (long long)w;
                        else if (l == to) own[j] += (long long)w;
                    }
                }
                if (tid == 0) own[i] = (long long)s_anew;
                __syncthreads();
            }
        }
        ++sweeps;
        if (tid == 0) s_moved = moved;
        __syncthreads();
        const int any = s_moved;
        __syncthreads();
        if (!any) break;
    }

    long long part = 0;                                                        // F of the result, literally
    for (long long j = tid; j < n; j += PSM_VI_THREADS) part -= 2 * pmdi_fixlog_L((unsigned long long)(own[j] + D), T);
    for (int g = tid; g < PSM_VI_G; g += PSM_VI_THREADS) part += pmdi_fixlog_sL(gsz[g], T);
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
    if (lane == 0) atomicAdd(&s_obj, (unsigned long long)part);
    __syncthreads();
    if (tid == 0) { moves_out[b] = moves; sweeps_out[b] = sweeps; objective_out[b] = (long long)s_obj; }
}

}  // namespace

// W: n x n uint32 work space; own: B n int64 work space.  labels [B][n], moves [B], sweeps [B], objective [B], flag [1] (zero
// before the launch) on the device.  1 <= n <= 65535, 1 <= B, D <= 2^31 - 1 and max_sweeps >= 1 are the caller's to check.
hipError_t pmdi_launch_psm_refine_vi(const int *counts, int K, long long n, int which, long long D, unsigned *W, long long *own,
                                     const int *start, long long B, long long ld, int max_sweeps, int *labels, long long *moves,
                                     int *sweeps, long long *objective, int *flag, hipStream_t stream)
{
    hipError_t e = pmdi_launch_psm_refine_build(counts, K, n, which, W, stream);
    if (e != hipSuccess) return e;
    const long long slab = 1LL << 20;                // starts per launch
    for (long long at = 0; at < B; at += slab) {
        const long long nb = B - at < slab ? B - at : slab;
        hipLaunchKernelGGL(psm_refine_vi_kernel, dim3((unsigned)nb), dim3(PSM_VI_THREADS), 0, stream, W, n, D, start + (size_t)at * ld, ld,
                           max_sweeps, labels + (size_t)at * n, own + (size_t)at * n, moves + at, sweeps + at, objective + at, flag);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

void pmdi_vi_log2_table_host(int *out)
{
    static const int table[PSM_VI_TABLE] = {
#include "pmdi_vi_log2_table.h"
    };
    for (int k = 0; k < PSM_VI_TABLE; ++k) out[k] = table[k];
}
