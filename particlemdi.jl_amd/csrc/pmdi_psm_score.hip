// pmdi_psm_score.hip -- candidate clusterings scored against the co-clustering counts (include/pmdi_hip.h,
// pmdi_psm_score_device): for every candidate c, agree = sum_{i>j} [c_i == c_j] w_ij and pairs = sum_{i>j} [c_i == c_j],
// and once per call total = sum_{i>j} w_ij.  Integer compares and integer sums only: exact in any order.
//
// Shape: LANES OWN CANDIDATES.  A workgroup (4 waves) takes a chunk of 64 candidates, one per lane, and walks 64 x 64
// tiles of the lower triangle.  Per tile it stages in LDS
//   * the w tile, read from HBM once per chunk (and, for the Overall matrix, summed over the K datasets once per chunk);
//     elements outside i > j, i < n are staged as 0,
//   * the row and the column labels of the 64 candidates, label-major ([obs][candidate], 65-int rows: the staging
//     writes and the reads are both conflict-free),
// then wave q takes rows 16 q .. 16 q + 15 in two blocks of 8: a lane keeps its candidate's 8 row labels in registers,
// reads one column label per column, and every w it tests is the same address in all lanes (an LDS broadcast).  A lane's
// sums are its own, so there is no cross-lane reduction; the 4 waves are combined through LDS at the very end and a
// workgroup issues 64 + 64 integer atomics for all the tiles it walked.
//
// The other shape (lanes own tile elements, candidates looped, one accumulator register per candidate of the chunk and
// a wave reduction per candidate at the end) saves the pairs += 1 of the inner loop, which becomes a scalar popcount of
// the compare mask, but pays 64 cross-lane reductions per workgroup, holds the chunk's accumulators in 64+ VGPRs and
// reads two labels per pair from LDS where this one reads one per 8 pairs.  It was not built.
#include <hip/hip_runtime.h>

#include "pmdi_internal.h"
#include "pmdi_psm_device.h"

namespace {

// WT = unsigned: the caller guarantees D = S (or S K for the Overall matrix) <= 2^22, so that
//   * a staged w (at most D when the counts are what they claim to be) fits 32 bits, and
//   * the partial sum `a` of one block of 8 rows x 64 columns is at most 512 * 2^22 = 2^31 < 2^32;
//   it is added to the 64-bit sum after every block.
// WT = unsigned long long: any D the interface admits (D P < 2^62): every w and every sum is 64 bits wide.
// npair (32 bits, both forms): a wave tests at most 16 x 64 pairs per tile and a workgroup walks at most
// 1024 * 1025 / 2 = 524800 tiles (n <= 65535), so a lane counts at most 1024 * 524800 < 2^30 pairs.
template <typename WT>
__global__ void __launch_bounds__(256) psm_score_kernel(const int *__restrict__ counts, int K, long long n, int which,
                                                        const int *__restrict__ cand, long long B, long long ld, unsigned n_tile_pairs,
                                                        int want_total, unsigned long long *__restrict__ agree_out,
                                                        unsigned long long *__restrict__ pairs_out, unsigned long long *__restrict__ total_out)
{
    __shared__ __attribute__((aligned(16))) WT wt[64][64];
    __shared__ int rl[64][PSM_LDL];
    __shared__ int cl[64][PSM_LDL];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);       // wave-uniform, and known to be: rows and branches go scalar
    const long long b0 = (long long)blockIdx.x * 64;
    int k_lo, k_hi;
    psm_k_range(which, K, k_lo, k_hi);
    unsigned long long agree = 0, tot = 0;
    unsigned npair = 0;

    for (unsigned p = blockIdx.y; p < n_tile_pairs; p += gridDim.y) {
        int bi, bj;
        psm_tile_pair_uniform(p, bi, bj);
        const long long i0 = (long long)bi * 64, j0 = (long long)bj * 64;
        // the w tile: a wave reads 64 consecutive ints of one row
#pragma unroll 4
        for (int rr = wave; rr < 64; rr += 4) {
            const long long i = i0 + rr, j = j0 + lane;
            WT w = 0;
            if (i < n && j < i) w = psm_w<WT>(counts, k_lo, k_hi, n, i, j);
            wt[rr][lane] = w;
            tot += w;
        }
        // the labels: a wave reads 64 consecutive labels of one candidate, twice (the tile's rows, the tile's columns)
        psm_stage_labels<true>(cand, B, ld, b0, n, wave, lane, rl, i0, cl, j0);
        __syncthreads();
#pragma unroll 1
        for (int rb = 0; rb < 2; ++rb) {
            const int r0 = wave * 16 + rb * 8;
            const long long ia = i0 + r0;
            if (ia >= n) break;
            if (bi > bj && ia + 7 < n) {                   // 8 rows x 64 columns, all of them pairs i > j
                int ri[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) ri[r] = rl[r0 + r][lane];
                WT a = 0;
#pragma unroll 2
                for (int j = 0; j < 64; j += 4) {
                    int cj[4];
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) cj[jj] = cl[j + jj][lane];
#pragma unroll
                    for (int r = 0; r < 8; ++r) psm_cmp_add4(&wt[r0 + r][j], ri[r], cj, a, npair);
                }
                agree += a;
            } else {                                       // a diagonal tile, or the last rows of the matrix
                for (int r = 0; r < 8; ++r) {
                    const long long i = ia + r;
                    if (i >= n) break;
                    const int jm = (int)((i - j0) < 64 ? (i - j0) : 64);       // columns j0 + j < i
                    const int rv = rl[r0 + r][lane];
                    WT a = 0;
                    for (int j = 0; j < jm; ++j) {
                        const bool eq = rv == cl[j][lane];
                        a += eq ? wt[r0 + r][j] : (WT)0;
                        npair += eq ? 1u : 0u;
                    }
                    agree += a;
                }
            }
        }
        __syncthreads();
    }

    // the 4 waves of a candidate, then one atomic per candidate and sum
    unsigned long long *red = (unsigned long long *)&wt[0][0];          // 3 * 256 of them: 6 KiB of the 16 or 32
    red[tid] = agree;
    red[256 + tid] = (unsigned long long)npair;
    red[512 + tid] = tot;
    __syncthreads();
    if (tid < 64 && b0 + tid < B) {
        atomicAdd(&agree_out[b0 + tid], red[tid] + red[64 + tid] + red[128 + tid] + red[192 + tid]);
        atomicAdd(&pairs_out[b0 + tid], red[256 + tid] + red[320 + tid] + red[384 + tid] + red[448 + tid]);
    }
    if (want_total && blockIdx.x == 0 && tid >= 64 && tid < 128) {      // every tile is staged once by the chunk-0 workgroups
        unsigned long long t = red[512 + lane] + red[576 + lane] + red[640 + lane] + red[704 + lane];
        for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
        if (lane == 0) atomicAdd(total_out, t);
    }
}

}  // namespace

// n <= 65535, 1 <= B, which and K are the caller's to check (pmdi_psm_score_device).  out: B agree, B pairs, 1 total, all
// zero before the first launch.  wide: D > 2^22 (see the kernel).
hipError_t pmdi_launch_psm_score(const int *counts, int K, long long n, int which, int wide, const int *cand, long long B, long long ld,
                                 unsigned long long *out, hipStream_t stream)
{
    const unsigned tile_pairs = psm_tile_pairs(n, 64);
    const long long slab = 1LL << 24;                // candidates per launch: 2^18 chunks in grid.x
    for (long long at = 0; at < B; at += slab) {
        const long long nb = B - at < slab ? B - at : slab;
        const unsigned chunks = (unsigned)((nb + 63) / 64);
        // about 16 workgroups per CU in all, chunk fastest: the workgroups that share a w tile run side by side
        unsigned slots = 4096u / chunks;
        if (slots < 1u) slots = 1u;
        if (slots > tile_pairs) slots = tile_pairs;
        const dim3 grid(chunks, slots);
        if (wide)
            hipLaunchKernelGGL(psm_score_kernel<unsigned long long>, grid, dim3(256), 0, stream, counts, K, n, which, cand + (size_t)at * ld, nb, ld,
                               tile_pairs, at == 0 ? 1 : 0, out + at, out + B + at, out + 2 * B);
        else
            hipLaunchKernelGGL(psm_score_kernel<unsigned>, grid, dim3(256), 0, stream, counts, K, n, which, cand + (size_t)at * ld, nb, ld,
                               tile_pairs, at == 0 ? 1 : 0, out + at, out + B + at, out + 2 * B);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
