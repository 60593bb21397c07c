// pmdi_psm_device.h -- what the posterior-similarity-matrix kernels share: the lower-triangle tile-pair index, the reader of a
// `which` matrix, the candidate-scoring pieces of pmdi_psm_score.hip / pmdi_psm_rowscore.hip, and the one body behind each pair
// (one-shot, accumulating) of counting kernels of pmdi_kernels.hip / pmdi_psm_acc.hip.  Integer compares, int8 products and
// integer sums only: exact by construction.  The tile-pair part is plain C++ and also compiles for the host
// (tests/test_psm_tile_pair_host.py); everything below it is device code.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define PSM_HD __host__ __device__
#else
#define PSM_HD
#endif

// ---- tile pairs of the lower triangle -----------------------------------------------------------------------------------
// Tile pair p = bi (bi + 1) / 2 + bj, 0 <= bj <= bi.  At most 1024 tile rows (n <= 65535, tiles at least 64 wide): p < 2^20,
// where the float square root is within one of the answer; the two loops of psm_tile_row make it exact from any estimate.
PSM_HD inline int psm_tile_row_estimate(unsigned p) { return (int)((sqrtf(8.0f * (float)p + 1.0f) - 1.0f) * 0.5f); }

PSM_HD inline int psm_tile_row(unsigned p, int b)        // the bi of tile pair p, from an estimate b >= -1
{
    while ((unsigned)b * (unsigned)(b + 1) / 2u > p) --b;
    while ((unsigned)(b + 1) * (unsigned)(b + 2) / 2u <= p) ++b;
    return b;
}

PSM_HD inline void psm_tile_pair(unsigned p, int &bi, int &bj)
{
    bi = psm_tile_row(p, psm_tile_row_estimate(p));
    bj = (int)(p - (unsigned)bi * (unsigned)(bi + 1) / 2u);
}

// tile pairs of an n x n matrix cut into tile x tile tiles: T (T + 1) / 2 (the host side of every grid that walks them)
inline unsigned psm_tile_pairs(long long n, int tile)
{
    const long long T = (n + tile - 1) / tile;
    return (unsigned)(T * (T + 1) / 2);
}

#if defined(__HIPCC__)

// psm_tile_pair for a workgroup-uniform p that a kernel loops over: the float detour leaves bi in a vector register, and with
// it every tile address of the loop body; this puts it back into a scalar one
__device__ __forceinline__ void psm_tile_pair_uniform(unsigned p, int &bi, int &bj)
{
    bi = __builtin_amdgcn_readfirstlane(psm_tile_row(p, psm_tile_row_estimate(p)));
    bj = (int)(p - (unsigned)bi * (unsigned)(bi + 1) / 2u);
}

// ---- the `which` matrix of counts [K][n][n] -------------------------------------------------------------------------------
// which < K: dataset `which`; which == K: the Overall matrix, the sum over the K datasets.  The guards (i > j, i != j, inside
// the matrix) are the callers': they differ.
__device__ __forceinline__ void psm_k_range(int which, int K, int &k_lo, int &k_hi)
{
    k_lo = which < K ? which : 0;
    k_hi = which < K ? which + 1 : K;
}

__device__ __forceinline__ int psm_count(const int *__restrict__ counts, int k, long long n, long long i, long long j)
{
    return counts[((size_t)k * n + i) * n + j];
}

template <typename WT>
__device__ __forceinline__ WT psm_w(const int *__restrict__ counts, int k_lo, int k_hi, long long n, long long i, long long j)
{
    WT w = 0;
    for (int k = k_lo; k < k_hi; ++k) w += (WT)(unsigned)psm_count(counts, k, n, i, j);
    return w;
}

// ---- candidate scoring (pmdi_psm_score.hip, pmdi_psm_rowscore.hip) -------------------------------------------------------
#define PSM_LDL 65        // ints per row of a label table: [obs][candidate], staging writes and reads both conflict-free

template <typename WT>
struct alignas(16) PsmW4 {
    WT v[4];
};

// labels x0 .. x0 + 63 (and, with TWO, y0 .. y0 + 63 into a second table) of candidates b0 .. b0 + 63 into label-major tables:
// wave q reads 64 consecutive labels of candidate q + 4 e; 0 beyond the B candidates or the n observations.  TWO is a template
// flag and not a test of ty: a null test of an LDS pointer is not folded away early enough, and the kernel's registers change.
template <bool TWO>
__device__ __forceinline__ void psm_stage_labels(const int *cand, long long B, long long ld, long long b0, long long n, int wave,
                                                 int lane, int (*tx)[PSM_LDL], long long x0, int (*ty)[PSM_LDL] = nullptr, long long y0 = 0)
{
#pragma unroll 4
    for (int e = 0; e < 16; ++e) {
        const int b = wave + 4 * e;
        int xv = 0, yv = 0;
        if (b0 + b < B) {
            const int *row = cand + (size_t)(b0 + b) * ld;
            if (x0 + lane < n) xv = row[x0 + lane];
            if (TWO && y0 + lane < n) yv = row[y0 + lane];
        }
        tx[lane][b] = xv;
        if (TWO) ty[lane][b] = yv;
    }
}

// One row of the 8-row x 4-column compare-and-add block: four consecutive w of an LDS row (16-byte aligned) against the row's
// label ri and the four column labels cj.  a and cnt are the caller's accumulators: psm_score_kernel passes the same pair for
// all 8 rows, psm_rowscore_kernel a pair per row.
template <typename WT, typename CT>
__device__ __forceinline__ void psm_cmp_add4(const WT *w, int ri, const int (&cj)[4], WT &a, CT &cnt)
{
    PsmW4<WT> w4 = *(const PsmW4<WT> *)w;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) asm volatile("" : "+v"(w4.v[jj]));     // one wide LDS read, not four guarded ones
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        const bool eq = ri == cj[jj];
        a += eq ? w4.v[jj] : (WT)0;
        cnt += eq ? (CT)1 : (CT)0;
    }
}

// ---- counting kernels (pmdi_kernels.hip: counts = tile; pmdi_psm_acc.hip: counts += tile) ----------------------------------
// Each __global__ wrapper says which tile and where it goes: (i0, j0) its first row and column, i_end the end of the rows it may
// read and write (the columns end at n); the output holds out_rows rows of n ints per dataset, the first of them row out_row0 of
// the matrix.  ACC: counts += tile, else counts = tile.
//
// How the staged values of one round get into LDS is the body's STAGE parameter, the staging rule:
//   Elem            the staged value's type
//   round<ROWS, COLS>(As, Bs, ...)    stages samples t0 .. t0 + ROWS - 1 of the tile's COLS rows (from i0) into As and of its COLS
//                   columns (from j0) into Bs; what lies beyond the matrix or the samples is staged as a padding value that is never
//                   equal to anything staged on the other side (MFMA bodies: outside every 32-label block in use)
// PsmStageLabel: the label of dataset k -- the per-dataset counts.  One byte per lane and step, rows and columns guarded apart.
struct PsmStageLabel {
    typedef unsigned char Elem;
    int k;
    template <int ROWS, int COLS>
    __device__ __forceinline__ void round(Elem (*As)[COLS], Elem (*Bs)[COLS], const unsigned char *__restrict__ samples, long long t0,
                                          long long S, int K, long long n, long long i0, long long j0, long long i_end, int lc, int lt) const
    {
#pragma unroll 4
        for (int tt = lt; tt < ROWS; tt += 256 / COLS) {
            const long long t = t0 + tt;
            unsigned char av = 255, bv = 254;                    // padding: never equal to anything on the other side
            if (t < S) {
                const unsigned char *row = samples + ((size_t)t * K + k) * n;
                if (i0 + lc < i_end) av = row[i0 + lc];
                if (j0 + lc < n) bv = row[j0 + lc];
            }
            As[tt][lc] = av; Bs[tt][lc] = bv;
        }
    }
};

// PsmStageFused: the label the NM datasets mem[] share (a group of fewer repeats its first member), or "nothing" when they do not
// all agree -- the fused counts of pmdi_fusion.hip.  E = unsigned char for the MFMA bodies, where the padding bytes already are
// "nothing" (an all-zero one-hot row); E = unsigned short for the byte compares, where every byte 0..255 may be a label and the
// fused flag needs a bit of its own: 0x100 / 0x200 lie above all of them.  Every address is clamped into the batch and the guards
// select afterwards, so no load sits under a branch: the 2 NM loads of each of four steps are in flight together.
template <typename E, int NM>
struct PsmStageFused {
    typedef E Elem;
    static constexpr Elem pad_a = sizeof(E) == 1 ? 255 : 0x100, pad_b = sizeof(E) == 1 ? 254 : 0x200;
    int mem[NM];
    __device__ __forceinline__ explicit PsmStageFused(unsigned mask)       // mask: workgroup-uniform, 2 .. NM bits set
    {
        const int first = __builtin_ctz(mask);
#pragma unroll
        for (int j = 0; j < NM; ++j) {
            mem[j] = mask ? __builtin_ctz(mask) : first;
            mask &= mask - 1;
        }
    }
    template <int ROWS, int COLS>
    __device__ __forceinline__ void round(Elem (*As)[COLS], Elem (*Bs)[COLS], const unsigned char *__restrict__ samples, long long t0,
                                          long long S, int K, long long n, long long i0, long long j0, long long i_end, int lc, int lt) const
    {
        const bool in_a = i0 + lc < i_end, in_b = j0 + lc < n;
        const long long xa = in_a ? i0 + lc : i0, xb = in_b ? j0 + lc : j0;       // (i0 < i_end <= n and j0 < n: both inside)
#pragma unroll 4
        for (int tt = lt; tt < ROWS; tt += 256 / COLS) {
            const long long t = t0 + tt;
            const unsigned char *row = samples + (size_t)(t < S ? t : S - 1) * K * n;
            unsigned char a[NM], b[NM];
#pragma unroll
            for (int j = 0; j < NM; ++j) { a[j] = row[(size_t)mem[j] * n + xa]; b[j] = row[(size_t)mem[j] * n + xb]; }
            bool fa = in_a && t < S, fb = in_b && t < S;
#pragma unroll
            for (int j = 1; j < NM; ++j) { fa &= a[j] == a[0]; fb &= b[j] == b[0]; }
            As[tt][lc] = fa ? (Elem)a[0] : pad_a; Bs[tt][lc] = fb ? (Elem)b[0] : pad_b;
        }
    }
};

// four consecutive staged values of an LDS row as one read
__device__ __forceinline__ void psm_unpack4(const unsigned char *p, unsigned (&v)[4])
{
    const unsigned v4 = *(const unsigned *)p;
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = (v4 >> (8 * r)) & 0xffu;
}

__device__ __forceinline__ void psm_unpack4(const unsigned short *p, unsigned (&v)[4])
{
    const uint2 v4 = *(const uint2 *)p;
    v[0] = v4.x & 0xffffu; v[1] = v4.x >> 16; v[2] = v4.y & 0xffffu; v[3] = v4.y >> 16;
}

// Byte compares on the vector ALUs (any label 0..255).  One workgroup = a 64 x 64 tile of (row i, column j) pairs of matrix k;
// 256 lanes, 4 x 4 pairs each.  The staged values of 64 samples for the tile's 64 rows and 64 columns are kept in LDS (sample-major,
// so a lane reads its 4 row values and 4 column values as one dword, or two, each).
#define PSM_TT 64
template <bool ACC, typename STAGE>
__device__ __forceinline__ void psm_count_body(const STAGE stage, const unsigned char *__restrict__ samples, long long S, int K,
                                               long long n, int k, long long i0, long long j0, long long i_end, long long out_rows,
                                               long long out_row0, int *__restrict__ counts)
{
    typedef typename STAGE::Elem Elem;
    __shared__ __attribute__((aligned(16))) Elem As[PSM_TT][64];
    __shared__ __attribute__((aligned(16))) Elem Bs[PSM_TT][64];
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    int acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0;
    const int lc = tid & 63, lt = tid >> 6;                 // staging: column of the tile, sample row mod 4
    for (long long t0 = 0; t0 < S; t0 += PSM_TT) {
        stage.template round<PSM_TT, 64>(As, Bs, samples, t0, S, K, n, i0, j0, i_end, lc, lt);
        __syncthreads();
#pragma unroll 8
        for (int tt = 0; tt < PSM_TT; ++tt) {
            unsigned a[4], b[4];
            psm_unpack4(&As[tt][ty * 4], a);
            psm_unpack4(&Bs[tt][tx * 4], b);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] += (a[r] == b[c]) ? 1 : 0;
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long i = i0 + ty * 4 + r;
        if (i >= i_end) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const long long j = j0 + tx * 4 + c;
            if (j >= n) continue;
            int &o = counts[((size_t)k * out_rows + (i - out_row0)) * n + j];
            if (ACC) o += acc[r][c];
            else o = acc[r][c];
        }
    }
}

// The matrix cores, for labels known to be < 32 * NKB: with one-hot rows A[i][(t, l)] = [samples[t][i] == l] the counts are
// A * A^T, an int8 GEMM whose K dimension is (sample, label); one v_mfma_i32_32x32x32_i8 covers one sample x 32 labels for a
// 32 x 32 tile of pairs.  Workgroup = 4 waves = a 128 x 128 tile, each wave a 64 x 64 quadrant (4 accumulator tiles).  The
// one-hot fragments are built in registers from the staged label bytes: lane (r = l & 31, h = l >> 5) holds 16 of the 32
// k-values of row r; which 16 does not matter as long as A and B use the same rule, because the sum over k does not depend on
// their order and the hardware pairs A's and B's k by the same (h, byte) position.  The padding bytes lie outside every
// 32-label block used.  C/D layout: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5).
typedef int psm_v4i __attribute__((ext_vector_type(4)));
typedef int psm_v16i __attribute__((ext_vector_type(16)));

__device__ __forceinline__ psm_v4i psm_onehot(int label, int kb, int h)
{
    const unsigned x = (unsigned)(label - 32 * kb - 16 * h);      // byte position among this lane's 16 k-values
    const unsigned bit = (x < 16u) ? (1u << ((x & 3u) * 8u)) : 0u;
    const unsigned dw = x >> 2;
    psm_v4i f;
    f.x = (dw == 0u) ? (int)bit : 0; f.y = (dw == 1u) ? (int)bit : 0; f.z = (dw == 2u) ? (int)bit : 0; f.w = (dw == 3u) ? (int)bit : 0;
    return f;
}

#define PSM_MT 32       // samples staged per round
template <int NKB, bool ACC, typename STAGE>
__device__ __forceinline__ void psm_count_mfma_body(const STAGE stage, const unsigned char *__restrict__ samples, long long S, int K,
                                                    long long n, int k, long long i0, long long j0, long long i_end, long long out_rows,
                                                    long long out_row0, int *__restrict__ counts)
{
    static_assert(sizeof(typename STAGE::Elem) == 1, "the one-hot fragments are built from staged bytes");
    __shared__ __attribute__((aligned(16))) unsigned char As[PSM_MT][128];
    __shared__ __attribute__((aligned(16))) unsigned char Bs[PSM_MT][128];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wy = wave >> 1, wx = wave & 1;                   // this wave's 64 x 64 quadrant
    const int r = lane & 31, h = lane >> 5;
    psm_v16i acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0;
    const int lc = tid & 127, lt = tid >> 7;                   // staging: column of the tile, sample row mod 2
    for (long long t0 = 0; t0 < S; t0 += PSM_MT) {
        stage.template round<PSM_MT, 128>(As, Bs, samples, t0, S, K, n, i0, j0, i_end, lc, lt);
        __syncthreads();
#pragma unroll 2
        for (int tt = 0; tt < PSM_MT; ++tt) {
            const int a0 = As[tt][wy * 64 + r], a1 = As[tt][wy * 64 + 32 + r];
            const int b0 = Bs[tt][wx * 64 + r], b1 = Bs[tt][wx * 64 + 32 + r];
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) {
                const psm_v4i fa0 = psm_onehot(a0, kb, h), fa1 = psm_onehot(a1, kb, h);
                const psm_v4i fb0 = psm_onehot(b0, kb, h), fb1 = psm_onehot(b1, kb, h);
                acc[0][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa0, fb0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa0, fb1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa1, fb0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa1, fb1, acc[1][1], 0, 0, 0);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const long long i = i0 + wy * 64 + a * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                const long long j = j0 + wx * 64 + b * 32 + r;
                if (i < i_end && j < n) {
                    int &o = counts[((size_t)k * out_rows + (i - out_row0)) * n + j];
                    if (ACC) o += acc[a][b][e];
                    else o = acc[a][b][e];
                }
            }
}

#endif  // __HIPCC__
