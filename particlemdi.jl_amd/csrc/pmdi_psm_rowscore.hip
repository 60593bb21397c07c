// pmdi_psm_rowscore.hip -- per-observation scores of candidate clusterings against the co-clustering counts
// (include/pmdi_hip.h, pmdi_psm_rowscore_device): for every candidate c and observation i
//   own[i] = sum_{j != i, c_j == c_i} w_ij   and   size[i] = #{j : c_j == c_i}  (i itself included),
// and once per call rowtotal[i] = sum_{j != i} w_ij, with w_ij = w_ji read from the lower triangle only.  Integer compares
// and integer sums: exact in any order.
//
// Shape: LANES OWN CANDIDATES, ONE WORKGROUP OWNS A TILE-ROW.  The shape of psm_score_kernel (pmdi_psm_score.hip) with the
// sums kept per (candidate, row).  A workgroup (4 waves) takes a chunk of 64 candidates, one per lane, and ONE block of 64
// rows, and walks all the 64-column tiles of that block of rows: the tiles left of the diagonal as they are stored, the
// tiles right of it as the transpose of their mirror image (read along the stored rows, so every HBM read is coalesced,
// and turned round on the way into LDS).  Wave q owns rows 16 q .. 16 q + 15: a lane keeps its candidate's 16 row labels
// and the 16 + 16 sums in registers for the whole walk, reads one column label per column from LDS, and every w it tests
// is the same LDS address in all lanes (a broadcast).  Every output element has exactly one writer: no atomics, no zeroing
// pass, and the outputs leave through LDS so that a wave writes 64 consecutive rows of one candidate.
//
// The other shape the lower triangle allows (walk only the tiles with bi >= bj, as psm_score_kernel does, and let a tile
// with bi > bj add to the rows of bi and to the rows of bj) tests half as many pairs, but the second direction sums over
// the tile's ROWS: 64 more running sums per lane (or an LDS read-modify-write per test), and 2 x 64 x 64 64-bit atomics per
// tile and chunk into `own` -- 16 bytes of atomic traffic for every 64 pair tests, against none here.  It was not built.
#include <hip/hip_runtime.h>

#include "pmdi_internal.h"
#include "pmdi_psm_device.h"

namespace {

// w rows are padded by 16 bytes: the 16-byte reads of four consecutive w stay aligned, and the turned-round staging of a
// mirrored tile (a wave writes one COLUMN) is a 4-way bank conflict, not a 32-way one
template <typename WT>
struct PsmRowShape {
    static constexpr int WS = 64 + 16 / (int)sizeof(WT);                   // 68 (32-bit) or 66 (64-bit) elements per row
    static constexpr int W_BYTES = 64 * WS * (int)sizeof(WT);              // 17 408 or 33 792
    static constexpr int L_BYTES = 64 * PSM_LDL * 4;                   // 16 640
    static constexpr int BYTES = W_BYTES + L_BYTES;                        // >= 64 * 65 * 8 = 33 280: the output staging fits
};

// WT = unsigned: the caller guarantees D = S (or S K for the Overall matrix) <= 2^22, so a staged w (at most D when the
//   counts are what they claim to be) fits 32 bits and the sum of one row over one tile is at most 64 * 2^22 = 2^28; it is
//   added to the 64-bit sum after every tile.
// WT = unsigned long long: any D the interface admits (D (n - 1) < 2^62).
// grid: x = chunk of 64 candidates (fastest: the workgroups that share a block of rows run side by side), y = block of rows.
template <typename WT>
__global__ void __launch_bounds__(256) psm_rowscore_kernel(const int *__restrict__ counts, int K, long long n, int which,
                                                           const int *__restrict__ cand, long long B, long long ld, int first_launch,
                                                           unsigned long long *__restrict__ own_out, int *__restrict__ size_out,
                                                           unsigned long long *__restrict__ rowtotal_out)
{
    const bool want_total = first_launch && blockIdx.x == 0;        // every tile-row is walked by one chunk-0 workgroup
    constexpr int WS = PsmRowShape<WT>::WS;
    __shared__ __attribute__((aligned(16))) unsigned char smem[PsmRowShape<WT>::BYTES];
    WT(*wt)[WS] = (WT(*)[WS])smem;
    int(*cl)[PSM_LDL] = (int(*)[PSM_LDL])(smem + PsmRowShape<WT>::W_BYTES);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long b0 = (long long)blockIdx.x * 64;
    const int bi = blockIdx.y;
    const int T = (int)((n + 63) / 64);
    const long long i0 = (long long)bi * 64;
    int k_lo, k_hi;
    psm_k_range(which, K, k_lo, k_hi);
    const int r0 = wave * 16;

    // the row labels, once: through the column-label buffer into registers
    // (psm_stage_labels' loop, spelled out: through the function this one read costs the kernel two more VGPRs)
#pragma unroll 4
    for (int e = 0; e < 16; ++e) {
        const int b = wave + 4 * e;
        int rv = 0;
        if (b0 + b < B && i0 + lane < n) rv = cand[(size_t)(b0 + b) * ld + i0 + lane];
        cl[lane][b] = rv;
    }
    __syncthreads();
    int ri[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) ri[r] = cl[r0 + r][lane];
    __syncthreads();

    unsigned long long own[16];
    int cnt[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { own[r] = 0; cnt[r] = 0; }
    unsigned long long rtot = 0;                                   // threads 0..63 of the chunk-0 workgroups: row i0 + tid

    for (int bj = 0; bj < T; ++bj) {
        const long long j0 = (long long)bj * 64;
        // the w tile (rows i0.., columns j0..), 0 on the diagonal and outside the matrix
        if (bj < bi) {                                             // stored as it is read
#pragma unroll 4
            for (int rr = wave; rr < 64; rr += 4) {
                const long long i = i0 + rr, j = j0 + lane;
                WT w = 0;
                if (i < n) w = psm_w<WT>(counts, k_lo, k_hi, n, i, j);
                wt[rr][lane] = w;
            }
        } else if (bj > bi) {                                      // the mirror image: stored row j, columns i0..
#pragma unroll 4
            for (int rr = wave; rr < 64; rr += 4) {
                const long long j = j0 + rr, i = i0 + lane;
                WT w = 0;
                if (j < n && i < n) w = psm_w<WT>(counts, k_lo, k_hi, n, j, i);
                wt[lane][rr] = w;
            }
        } else {                                                   // the diagonal tile: both halves from below the diagonal
            for (int rr = wave; rr < 64; rr += 4) {
                const long long i = i0 + rr, j = j0 + lane;
                WT w = 0;
                if (i < n && j < n && i != j) w = psm_w<WT>(counts, k_lo, k_hi, n, i > j ? i : j, i > j ? j : i);
                wt[rr][lane] = w;
            }
        }
        // the column labels: a wave reads 64 consecutive labels of one candidate
        psm_stage_labels<false>(cand, B, ld, b0, n, wave, lane, cl, j0);
        __syncthreads();
        if (want_total && tid < 64) {                              // one row per thread, columns rotated: no bank conflict
            unsigned long long t = 0;
            for (int j = 0; j < 64; ++j) t += (unsigned long long)wt[tid][(j + tid) & 63];
            rtot += t;
        }
        const int jm = (int)(n - j0 < 64 ? n - j0 : 64);           // columns of this tile inside the matrix
        if (jm == 64) {
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) {
                WT a[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) a[r] = 0;
#pragma unroll 2
                for (int j = 0; j < 64; j += 4) {
                    int cj[4];
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) cj[jj] = cl[j + jj][lane];
#pragma unroll
                    for (int r = 0; r < 8; ++r) psm_cmp_add4(&wt[r0 + rb * 8 + r][j], ri[rb * 8 + r], cj, a[r], cnt[rb * 8 + r]);
                }
#pragma unroll
                for (int r = 0; r < 8; ++r) own[rb * 8 + r] += a[r];
            }
        } else {                                                   // the last tile of the row: columns beyond n carry no label
            for (int j = 0; j < jm; ++j) {
                const int cj = cl[j][lane];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const bool eq = ri[r] == cj;
                    own[r] += eq ? (unsigned long long)wt[r0 + r][j] : 0ull;
                    cnt[r] += eq ? 1 : 0;
                }
            }
        }
        __syncthreads();
    }

    if (want_total && tid < 64 && i0 + tid < n) rowtotal_out[i0 + tid] = rtot;

    // out through LDS, [candidate][row]: a wave then writes 64 consecutive rows of one candidate
    unsigned long long(*ob)[PSM_LDL] = (unsigned long long(*)[PSM_LDL])smem;
#pragma unroll
    for (int r = 0; r < 16; ++r) ob[lane][r0 + r] = own[r];
    __syncthreads();
    for (int e = 0; e < 16; ++e) {
        const int b = wave + 4 * e;
        if (b0 + b < B && i0 + lane < n) own_out[(size_t)(b0 + b) * n + i0 + lane] = ob[b][lane];
    }
    __syncthreads();
    int(*sb)[PSM_LDL] = (int(*)[PSM_LDL])smem;
#pragma unroll
    for (int r = 0; r < 16; ++r) sb[lane][r0 + r] = cnt[r];
    __syncthreads();
    for (int e = 0; e < 16; ++e) {
        const int b = wave + 4 * e;
        if (b0 + b < B && i0 + lane < n) size_out[(size_t)(b0 + b) * n + i0 + lane] = sb[b][lane];
    }
}

}  // namespace

// 1 <= n <= 65535, 1 <= B, which and K are the caller's to check (pmdi_psm_rowscore_device).  own [B][n], size [B][n],
// rowtotal [n]: every element is written exactly once, so nothing has to be zeroed first.  wide: D > 2^22 (see the kernel).
hipError_t pmdi_launch_psm_rowscore(const int *counts, int K, long long n, int which, int wide, const int *cand, long long B, long long ld,
                                    unsigned long long *own, int *size, unsigned long long *rowtotal, hipStream_t stream)
{
    const unsigned T = (unsigned)((n + 63) / 64);
    const long long slab = 1LL << 24;                // candidates per launch: 2^18 chunks in grid.x
    for (long long at = 0; at < B; at += slab) {
        const long long nb = B - at < slab ? B - at : slab;
        const dim3 grid((unsigned)((nb + 63) / 64), T);
        if (wide)
            hipLaunchKernelGGL(psm_rowscore_kernel<unsigned long long>, grid, dim3(256), 0, stream, counts, K, n, which,
                               cand + (size_t)at * ld, nb, ld, at == 0 ? 1 : 0, own + (size_t)at * n, size + (size_t)at * n, rowtotal);
        else
            hipLaunchKernelGGL(psm_rowscore_kernel<unsigned>, grid, dim3(256), 0, stream, counts, K, n, which, cand + (size_t)at * ld, nb, ld,
                               at == 0 ? 1 : 0, own + (size_t)at * n, size + (size_t)at * n, rowtotal);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
