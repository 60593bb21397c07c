// pmdi_partdist_refine.hip -- coordinate descent of the Monte-Carlo expected loss against the sampled clusterings themselves
// (include/pmdi_hip.h, pmdi_partition_refine_device): F(c) = R sum_g M(a_g) - 2 sum_r sum_gh M(n^r_gh) with M(x) = x L(x) (VI, the
// fixed-point logarithm of pmdi_fixlog.h) or x (x - 1) / 2 (Binder).  Every gain is an exact int64, so the descent is the same on
// every run and on every machine.  Visiting order, ranking of the options and the tie rule are those of pmdi_psm_refine.hip.
//   partref_transpose_kernel  the draw bytes [R][np] of pmdi_partition_rows_device into [n][R], so that the R labels of one
//                             observation are contiguous; a byte >= Gd before column n raises the flag and goes out as 0, so
//                             nothing is indexed by it
//   partref_kernel<loss>      ONE PERSISTENT WORKGROUP PER START (16 waves).  Its contingency tables live in global memory as
//                             uint16 [r][h][g], g fastest and padded to Gp = a power of two >= gcap: for a fixed r and
//                             h = s_r(i) the slots are one contiguous run of 2 Gp bytes.  Every cell of draw row r is written
//                             by thread r % 1024 only, here and when the tables are first formed: no atomics on global memory.
// A visit of i is three phases:
//   1. scoring.  The live slots are listed in LDS in ascending order (wave 0 lists them anew when a group appears or vanishes).
//      With Gq = the power of two >= their number, thread t owns the (t % Gq)-th live slot and the stripe t / Gq of draw rows
//      r = stripe, stripe + 1024 / Gq, ...: it reads h = s_r(i) (one byte, the same for the lanes of a stripe) and the cell
//      (r, h, slot), one less for i's own group, and adds d(cell) = M(cell + 1) - M(cell) privately; the stripes of a wave are
//      folded with shuffles, those of different waves go through LDS (64-bit integer adds: any order);
//   2. wave 0 forms score(g) = 2 sum_r d - R d(a_g), reduces (score, slot) with shuffles under the tie rule and decides;
//   3. only when i moved, thread r % 1024 takes one from cell (r, h, old) and adds one to cell (r, h, new).
// Two barriers per visit, a third on a move.  i is never physically taken out of its group: the scoring reads its cell as one
// less.  LDS: the partial sums 8 KiB, the table of L 8 KiB, the group sizes 1 KiB, the list 256 bytes.
// A visit reads R runs of at most 2 Gp bytes, each in a cache line of its own: at the headline shape (R = 12 288, Gp = 64) 1.5 MB of
// lines per visit from tables of R Gd Gp 2 bytes per start, far beyond L2.
//
// Not built: d(x) from a table of n int64 in place of two evaluations of L per cell; tables in a layout that follows the live
// slots rather than gcap; the tables formed by a grid-wide kernel rather than by the start's own workgroup.
#include <hip/hip_runtime.h>

#include "pmdi_fixlog.h"
#include "pmdi_internal.h"

namespace {

#define PR_THREADS 1024
#define PR_WAVES (PR_THREADS / 64)
#define PR_SLOTS 256      // Gp at most: gcap <= 255
#define PR_DEPTH 8        // cells a thread gathers before it uses the first
#define PR_BATCH 4        // draw rows a thread updates side by side

__device__ const int pr_table[PMDI_FIXLOG_TABLE] = {
#include "pmdi_vi_log2_table.h"
};

__global__ void __launch_bounds__(256) partref_transpose_kernel(const unsigned char *__restrict__ bytes, long long R, long long n, int np, int Gd,
                                                                unsigned char *__restrict__ out, int *__restrict__ flag)
{
    __shared__ unsigned char tile[64][65];
    const int x = threadIdx.x & 63, y = threadIdx.x >> 6;
    const long long r0 = (long long)blockIdx.x * 64, i0 = (long long)blockIdx.y * 64;
    int bad = 0;
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
        const long long r = r0 + y + 4 * k, i = i0 + x;
        if (r < R && i < n) {
            unsigned char v = bytes[r * np + i];
            if (v >= Gd) { bad = 1; v = 0; }
            tile[y + 4 * k][x] = v;
        }
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
        const long long i = i0 + y + 4 * k, r = r0 + x;
        if (i < n && r < R) out[i * R + r] = tile[x][y + 4 * k];
    }
    if (bad) atomicOr(flag, 2);
}

// M(x) and d(x) = M(x + 1) - M(x) for 0 <= x <= 65535; d(0) = 0 in both losses
template <int LOSS>
__device__ __forceinline__ unsigned long long pr_M(unsigned x, const int *T)
{
    return LOSS ? pmdi_fixlog_vL32(x, T) : (unsigned long long)((x * (x - 1u)) >> 1);       // x = 0: the product is 0
}

template <int LOSS>
__device__ __forceinline__ long long pr_d(unsigned x, const int *T)
{
    return LOSS ? (long long)(pmdi_fixlog_vL32(x + 1u, T) - pmdi_fixlog_vL32(x, T)) : (long long)x;
}

__device__ __forceinline__ int pr_log2_ceil(int v) { return v <= 1 ? 0 : 32 - __clz(v - 1); }

// The slots with members, ascending, into list[]; their number.  One whole wave calls it.
__device__ __forceinline__ int pr_list_live(const int *gsz, int gcap, unsigned char *list, int lane)
{
    int count = 0;
    for (int base = 0; base < gcap; base += 64) {
        const int s = base + lane;
        const bool on = s < gcap && gsz[s] > 0;
        const unsigned long long mask = __ballot(on);
        if (on) list[count + __popcll(mask & ((1ull << lane) - 1ull))] = (unsigned char)s;
        count += __popcll(mask);
    }
    return count;
}

template <int LOSS>
__global__ void __launch_bounds__(PR_THREADS) partref_kernel(const unsigned char *__restrict__ dT, long long R, int Gd, long long n,
                                                             const int *__restrict__ start, long long ld, int gcap, int lgp, int max_sweeps,
                                                             unsigned short *tables, long long cells, int *labels,
                                                             long long *__restrict__ moves_out, int *__restrict__ sweeps_out,
                                                             int *__restrict__ converged_out, long long *__restrict__ marginal_out,
                                                             long long *__restrict__ joint_out, int *__restrict__ flag)
{
    __shared__ unsigned long long part[PR_THREADS];      // [wave or stripe][slot] partial sums of d
    __shared__ int T[PMDI_FIXLOG_TABLE];
    __shared__ int gsz[PR_SLOTS];
    __shared__ unsigned long long s_joint;
    __shared__ unsigned char live_slot[PR_SLOTS];        // the live slots, ascending
    __shared__ int s_live, s_bad, s_moved, s_to;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long b = blockIdx.x;
    int *lab = labels + (size_t)b * n;
    unsigned short *tab = tables + (size_t)b * cells;
    const int *st = start + (size_t)b * ld;

    for (int g = tid; g < PR_SLOTS; g += PR_THREADS) gsz[g] = 0;
    for (int k = tid; k < PMDI_FIXLOG_TABLE; k += PR_THREADS) T[k] = pr_table[k];
    if (tid == 0) { s_live = 0; s_bad = 0; s_moved = 0; s_to = -1; s_joint = 0; }
    __syncthreads();
    {
        int bad = 0;
        for (long long j = tid; j < n; j += PR_THREADS) {
            const int v = st[j];
            if ((unsigned)v >= (unsigned)gcap) bad = 1;
            else atomicAdd(&gsz[v], 1);
            lab[j] = v;
        }
        if (bad) s_bad = 1;
    }
    __syncthreads();
    if (s_bad) {                                                   // workgroup-uniform: a start label outside the slot range
        if (tid == 0) {
            atomicOr(flag, 1);
            moves_out[b] = 0; sweeps_out[b] = 0; converged_out[b] = 0; marginal_out[b] = 0; joint_out[b] = 0;
        }
        return;
    }

    // the tables of the start (zero before the launch): the cells of row r by thread r % PR_THREADS
    // (four rows of a thread at a time: their cells are distinct, so the four loads go out before the four stores)
    for (long long r0 = tid; r0 < R; r0 += PR_BATCH * PR_THREADS)
        for (long long i = 0; i < n; ++i) {
            const int g = lab[i];
            unsigned short *cell[PR_BATCH];
            unsigned v[PR_BATCH];
#pragma unroll
            for (int u = 0; u < PR_BATCH; ++u) {
                const long long r = r0 + (long long)u * PR_THREADS;
                cell[u] = r < R ? tab + ((((size_t)r * Gd + dT[(size_t)i * R + r]) << lgp) + g) : nullptr;
            }
#pragma unroll
            for (int u = 0; u < PR_BATCH; ++u) v[u] = cell[u] ? *cell[u] : 0u;
#pragma unroll
            for (int u = 0; u < PR_BATCH; ++u)
                if (cell[u]) *cell[u] = (unsigned short)(v[u] + 1u);
        }

    // wave 0 keeps these, uniform over its lanes
    int live = 0;
    if (wave == 0) {
        live = pr_list_live(gsz, gcap, live_slot, lane);
        if (lane == 0) s_live = live;
    }
    long long moves = 0;
    int sweeps = 0, last_moved = 1;
    __syncthreads();

    for (int sweep = 0; sweep < max_sweeps; ++sweep) {
        int moved = 0;
        for (long long i = 0; i < n; ++i) {
            const unsigned char *col = dT + (size_t)i * R;
            const int cur = lab[i];
            const int nlive = s_live;                                          // workgroup-uniform; next written after the next barrier
            const int lgq = pr_log2_ceil(nlive), gq = 1 << lgq;
            const int at = tid & (gq - 1), stripe = tid >> lgq, nstr = PR_THREADS >> lgq;
            long long acc = 0;
            if (at < nlive) {
                const int g = live_slot[at];
                const unsigned own = g == cur ? 1u : 0u;
                for (long long r0 = stripe; r0 < R; r0 += PR_DEPTH * nstr) {   // PR_DEPTH gathers in flight per thread
                    unsigned h[PR_DEPTH], x[PR_DEPTH];
#pragma unroll
                    for (int u = 0; u < PR_DEPTH; ++u) {
                        const long long r = r0 + (long long)u * nstr;
                        h[u] = r < R ? col[r] : 0u;
                    }
#pragma unroll
                    for (int u = 0; u < PR_DEPTH; ++u) {
                        const long long r = r0 + (long long)u * nstr;
                        x[u] = own;                                            // past R: d(0) = 0
                        if (r < R) x[u] = tab[(((size_t)r * Gd + h[u]) << lgp) + g];
                    }
#pragma unroll
                    for (int u = 0; u < PR_DEPTH; ++u) acc += pr_d<LOSS>(x[u] - own, T);      // i's own cell holds i: at least 1
                }
            }
            for (int off = 32; off >= gq; off >>= 1) acc += __shfl_xor(acc, off, 64);  // the stripes of one wave (gq < 64)
            if (lgq >= 6) part[tid] = (unsigned long long)acc;                 // = [stripe][at]
            else if (lane < gq) part[wave * gq + lane] = (unsigned long long)acc;
            __syncthreads();
            if (wave == 0) {
                const int rows = lgq >= 6 ? nstr : PR_WAVES;                   // partial sums per slot
                const int sz_cur = gsz[cur];
                const bool alone = sz_cur == 1;
                long long bg = 0, mine = 0;
                int bs = -1;
                bool has_cur = false;
                for (int a = lane; a < nlive; a += 64) {                       // ascending slots: a lane keeps its lowest best
                    const int s = live_slot[a];
                    const int sz = gsz[s] - (s == cur ? 1 : 0);
                    unsigned long long sum = 0;
                    for (int k = 0; k < rows; ++k) sum += part[k * gq + a];
                    const long long score = 2 * (long long)sum - R * pr_d<LOSS>((unsigned)sz, T);
                    if (s == cur) { mine = score; has_cur = true; }            // alone: every cell and the size are 0, the score is 0
                    else if (bs < 0 || score > bg) { bg = score; bs = s; }
                }
                const long long sc_cur = __shfl(mine, __ffsll((long long)__ballot(has_cur)) - 1, 64);       // cur is live: one lane has it
                for (int off = 32; off > 0; off >>= 1) {
                    const long long og = __shfl_xor(bg, off, 64);
                    const int os = __shfl_xor(bs, off, 64);
                    if (os >= 0 && (bs < 0 || og > bg || (og == bg && os < bs))) { bg = og; bs = os; }
                }
                long long tg = sc_cur;                                         // the current group first
                int target = cur;
                if (bs >= 0 && bg > tg) { target = bs; tg = bg; }
                if (!alone && live < gcap && 0 > tg) {                         // the new singleton: the lowest free slot
                    int f = PR_SLOTS;
                    for (int s = lane; s < gcap; s += 64)
                        if (gsz[s] == 0) { f = s; break; }
                    for (int off = 32; off > 0; off >>= 1) {
                        const int o = __shfl_xor(f, off, 64);
                        f = o < f ? o : f;
                    }
                    if (f < gcap) target = f;                                  // (live < gcap: there is one)
                }
                if (target != cur) {
                    const bool fresh = gsz[target] == 0;
                    if (lane == 0) {
                        gsz[cur] = sz_cur - 1; gsz[target] += 1; lab[i] = target;
                        s_to = target;
                    }
                    if (fresh || alone) {                                      // a group appeared or vanished: the list anew
                        live = pr_list_live(gsz, gcap, live_slot, lane);
                        if (lane == 0) s_live = live;
                    }
                    ++moves;
                    moved = 1;
                } else if (lane == 0) s_to = -1;
            }
            __syncthreads();
            const int to = s_to;                                               // workgroup-uniform; next written after the next barrier
            if (to >= 0) {
                for (long long r0 = tid; r0 < R; r0 += PR_BATCH * PR_THREADS) {   // distinct rows: the loads before the stores
                    unsigned short *cell[PR_BATCH];
                    unsigned from[PR_BATCH], into[PR_BATCH];
#pragma unroll
                    for (int u = 0; u < PR_BATCH; ++u) {
                        const long long r = r0 + (long long)u * PR_THREADS;
                        cell[u] = r < R ? tab + (((size_t)r * Gd + col[r]) << lgp) : nullptr;
                    }
#pragma unroll
                    for (int u = 0; u < PR_BATCH; ++u) {
                        from[u] = cell[u] ? cell[u][cur] : 0u;
                        into[u] = cell[u] ? cell[u][to] : 0u;
                    }
#pragma unroll
                    for (int u = 0; u < PR_BATCH; ++u)
                        if (cell[u]) {
                            cell[u][cur] = (unsigned short)(from[u] - 1u);
                            cell[u][to] = (unsigned short)(into[u] + 1u);
                        }
                }
                __syncthreads();
            }
        }
        ++sweeps;
        if (tid == 0) s_moved = moved;
        __syncthreads();
        last_moved = s_moved;
        __syncthreads();
        if (!last_moved) break;
    }

    unsigned long long joint = 0;                                              // the two sums of the result, literally
    for (long long k = tid; k < cells; k += PR_THREADS) joint += pr_M<LOSS>(tab[k], T);
    for (int off = 32; off > 0; off >>= 1) joint += __shfl_xor(joint, off, 64);
    if (lane == 0) atomicAdd(&s_joint, joint);
    __syncthreads();
    if (wave == 0) {
        unsigned long long marginal = 0;
        for (int g = lane; g < gcap; g += 64) marginal += pr_M<LOSS>((unsigned)gsz[g], T);
        for (int off = 32; off > 0; off >>= 1) marginal += __shfl_xor(marginal, off, 64);
        if (lane == 0) {
            moves_out[b] = moves; sweeps_out[b] = sweeps; converged_out[b] = last_moved ? 0 : 1;
            marginal_out[b] = (long long)marginal; joint_out[b] = (long long)s_joint;
        }
    }
}

}  // namespace

// draw_bytes [R][np] as pmdi_launch_partition_rows writes them; dT = n R bytes and tables = B cells uint16 of work space, cells =
// R Gd << lgp, lgp = log2 of the power of two >= gcap, the tables zero before the launch; labels [B][n], moves, marginal, joint [B]
// int64, sweeps, converged [B] int32 and flag [1] (zero before the launch; 1 = a start label, 2 = a draw byte) on the device.
// The limits of pmdi_partition_refine_device are the caller's to check.
hipError_t pmdi_launch_partition_refine(const unsigned char *draw_bytes, long long R, int Gd, long long n, unsigned char *dT,
                                        unsigned short *tables, int lgp, const int *start, long long B, long long ld, int gcap, int loss,
                                        int max_sweeps, int *labels, long long *moves, int *sweeps, int *converged, long long *marginal,
                                        long long *joint, int *flag, hipStream_t stream)
{
    const int np = (int)((n + 31) / 32 * 32);
    hipLaunchKernelGGL(partref_transpose_kernel, dim3((unsigned)((R + 63) / 64), (unsigned)((n + 63) / 64)), dim3(256), 0, stream, draw_bytes, R,
                       n, np, Gd, dT, flag);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const long long cells = (R * Gd) << lgp;
    auto fn = loss ? partref_kernel<1> : partref_kernel<0>;
    const long long slab = 1LL << 20;                // starts per launch
    for (long long at = 0; at < B; at += slab) {
        const long long nb = B - at < slab ? B - at : slab;
        hipLaunchKernelGGL(fn, dim3((unsigned)nb), dim3(PR_THREADS), 0, stream, dT, R, Gd, n, start + (size_t)at * ld, ld, gcap, lgp, max_sweeps,
                           tables + (size_t)at * cells, cells, labels + (size_t)at * n, moves + at, sweeps + at, converged + at, marginal + at,
                           joint + at, flag);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
