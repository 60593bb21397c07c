// pmdi_psm_acc.hip -- the streaming PSM accumulator (include/pmdi_hip.h, pmdi_psm_acc_*): the accumulating counterparts of
// psm_count_kernel / psm_count_mfma_kernel (pmdi_kernels.hip), which stay as they are.  Two differences from those:
//   * counts += tile.  Every (dataset, tile) belongs to exactly one workgroup of a launch and the launches of one
//     accumulator are ordered on one stream, so this is a plain read-modify-write: no atomics.
//   * only the tiles with block-row >= block-column are computed (the counts are symmetric); grid.x walks the
//     T (T + 1) / 2 lower tile pairs, diagonal tiles are computed whole.  The strict upper triangle is filled once, by
//     psm_acc_mirror_kernel, when the counts are asked for.
// Integer compares, int8 products and int32 sums only: exact by construction.
#include <hip/hip_runtime.h>

#include "pmdi_internal.h"

namespace {

// tile pair p = bi (bi + 1) / 2 + bj, 0 <= bj <= bi.  At most 1024 tile rows (n <= 65535, 64-wide tiles): p < 2^20, where the
// float square root is within one of the answer; the two loops make it exact.
__device__ __forceinline__ void psm_acc_tile_pair(unsigned p, int &bi, int &bj)
{
    int b = (int)((sqrtf(8.0f * (float)p + 1.0f) - 1.0f) * 0.5f);
    while ((unsigned)b * (unsigned)(b + 1) / 2u > p) --b;
    while ((unsigned)(b + 1) * (unsigned)(b + 2) / 2u <= p) ++b;
    bi = b;
    bj = (int)(p - (unsigned)b * (unsigned)(b + 1) / 2u);
}

// Byte compares on the vector ALUs (any label 0..255): a 64 x 64 tile per workgroup, 4 x 4 pairs per lane, the labels of 64
// samples for the tile's rows and columns staged in LDS sample-major (psm_count_kernel's scheme).
#define PSM_ACC_TT 64
__global__ void __launch_bounds__(256) psm_acc_kernel(const unsigned char *__restrict__ samples, long long S, int K, long long n,
                                                      int *__restrict__ counts)
{
    __shared__ __attribute__((aligned(16))) unsigned char As[PSM_ACC_TT][64];
    __shared__ __attribute__((aligned(16))) unsigned char Bs[PSM_ACC_TT][64];
    const int k = blockIdx.y;
    int bi, bj;
    psm_acc_tile_pair(blockIdx.x, bi, bj);
    const long long i0 = (long long)bi * 64, j0 = (long long)bj * 64;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    int acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0;
    const int lc = tid & 63, lt = tid >> 6;                 // staging: column of the tile, sample row mod 4
    for (long long t0 = 0; t0 < S; t0 += PSM_ACC_TT) {
#pragma unroll 4
        for (int tt = lt; tt < PSM_ACC_TT; tt += 4) {
            const long long t = t0 + tt;
            unsigned char av = 255, bv = 254;                // padding: never equal to anything on the other side
            if (t < S) {
                const unsigned char *row = samples + ((size_t)t * K + k) * n;
                if (i0 + lc < n) av = row[i0 + lc];
                if (j0 + lc < n) bv = row[j0 + lc];
            }
            As[tt][lc] = av; Bs[tt][lc] = bv;
        }
        __syncthreads();
#pragma unroll 8
        for (int tt = 0; tt < PSM_ACC_TT; ++tt) {
            const unsigned a4 = *(const unsigned *)&As[tt][ty * 4];
            const unsigned b4 = *(const unsigned *)&Bs[tt][tx * 4];
            unsigned a[4], b[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) { a[r] = (a4 >> (8 * r)) & 0xffu; b[r] = (b4 >> (8 * r)) & 0xffu; }
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
        if (i >= n) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const long long j = j0 + tx * 4 + c;
            if (j < n) counts[((size_t)k * n + i) * n + j] += acc[r][c];
        }
    }
}

// The matrix cores, for labels known to be < 32 * NKB: with one-hot rows A[i][(t, l)] = [s_t[i] == l] the counts are A * A^T,
// an int8 GEMM whose K dimension is (sample, label); one v_mfma_i32_32x32x32_i8 covers one sample x 32 labels for a 32 x 32
// tile of pairs.  Workgroup = 4 waves = a 128 x 128 tile, each wave a 64 x 64 quadrant (4 accumulator tiles).  Lane
// (r = l & 31, h = l >> 5) holds 16 of the 32 k-values of row r; A and B use the same rule, and the sum over k does not
// depend on their order.  C/D layout: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5).
typedef int psm_acc_v4i __attribute__((ext_vector_type(4)));
typedef int psm_acc_v16i __attribute__((ext_vector_type(16)));

__device__ __forceinline__ psm_acc_v4i psm_acc_onehot(int label, int kb, int h)
{
    const unsigned x = (unsigned)(label - 32 * kb - 16 * h);      // byte position among this lane's 16 k-values
    const unsigned bit = (x < 16u) ? (1u << ((x & 3u) * 8u)) : 0u;
    const unsigned dw = x >> 2;
    psm_acc_v4i f;
    f.x = (dw == 0u) ? (int)bit : 0; f.y = (dw == 1u) ? (int)bit : 0; f.z = (dw == 2u) ? (int)bit : 0; f.w = (dw == 3u) ? (int)bit : 0;
    return f;
}

#define PSM_ACC_MT 32       // samples staged per round
// 4 waves per SIMD asked for: the read half of counts += tile (64 loads and their addresses per lane) would otherwise set the
// kernel's register count (106 VGPRs + 64 AGPRs, 2 waves per SIMD) where the sample loop lives on half of that.
template <int NKB>
__global__ void __launch_bounds__(256, 4) psm_acc_mfma_kernel(const unsigned char *__restrict__ samples, long long S, int K, long long n,
                                                           int *__restrict__ counts)
{
    __shared__ __attribute__((aligned(16))) unsigned char As[PSM_ACC_MT][128];
    __shared__ __attribute__((aligned(16))) unsigned char Bs[PSM_ACC_MT][128];
    const int k = blockIdx.y;
    int bi, bj;
    psm_acc_tile_pair(blockIdx.x, bi, bj);
    const long long i0 = (long long)bi * 128, j0 = (long long)bj * 128;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wy = wave >> 1, wx = wave & 1;                   // this wave's 64 x 64 quadrant
    const int r = lane & 31, h = lane >> 5;
    psm_acc_v16i acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0;
    const int lc = tid & 127, lt = tid >> 7;                   // staging: column of the tile, sample row mod 2
    for (long long t0 = 0; t0 < S; t0 += PSM_ACC_MT) {
#pragma unroll 4
        for (int tt = lt; tt < PSM_ACC_MT; tt += 2) {
            const long long t = t0 + tt;
            unsigned char av = 255, bv = 254;                  // padding: outside every 32-label block used
            if (t < S) {
                const unsigned char *row = samples + ((size_t)t * K + k) * n;
                if (i0 + lc < n) av = row[i0 + lc];
                if (j0 + lc < n) bv = row[j0 + lc];
            }
            As[tt][lc] = av; Bs[tt][lc] = bv;
        }
        __syncthreads();
#pragma unroll 2
        for (int tt = 0; tt < PSM_ACC_MT; ++tt) {
            const int a0 = As[tt][wy * 64 + r], a1 = As[tt][wy * 64 + 32 + r];
            const int b0 = Bs[tt][wx * 64 + r], b1 = Bs[tt][wx * 64 + 32 + r];
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) {
                const psm_acc_v4i fa0 = psm_acc_onehot(a0, kb, h), fa1 = psm_acc_onehot(a1, kb, h);
                const psm_acc_v4i fb0 = psm_acc_onehot(b0, kb, h), fb1 = psm_acc_onehot(b1, kb, h);
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
        for (int b = 0; b < 2; ++b) {
        #pragma unroll
            for (int e = 0; e < 16; ++e) {
                const long long i = i0 + wy * 64 + a * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                const long long j = j0 + wx * 64 + b * 32 + r;
                if (i < n && j < n) counts[((size_t)k * n + i) * n + j] += acc[a][b][e];
            }
        }
}

// counts[k][j][i] = counts[k][i][j] for i > j: a 64 x 64 tile of the lower triangle is read row-wise, transposed through LDS
// (65-int rows: no bank conflicts) and written row-wise into its mirror image.  A diagonal tile writes its own strict upper part.
__global__ void __launch_bounds__(256) psm_acc_mirror_kernel(int *__restrict__ counts, long long n)
{
    __shared__ int tile[64][65];
    const int k = blockIdx.y;
    int bi, bj;
    psm_acc_tile_pair(blockIdx.x, bi, bj);
    const long long i0 = (long long)bi * 64, j0 = (long long)bj * 64;
    int *c = counts + (size_t)k * n * n;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int rr = ty; rr < 64; rr += 4) {
        const long long i = i0 + rr, j = j0 + tx;
        tile[rr][tx] = (i < n && j < n) ? c[(size_t)i * n + j] : 0;
    }
    __syncthreads();
    for (int rr = ty; rr < 64; rr += 4) {
        const long long j = j0 + rr, i = i0 + tx;             // destination row j, column i: strictly above the diagonal only
        if (i < n && j < n && i > j) c[(size_t)j * n + i] = tile[tx][rr];
    }
}

// a[k][i][j] += b[k][i][j] for j <= i (the other half of b is never read; the other half of a is the mirror kernel's)
__global__ void __launch_bounds__(256) psm_acc_merge_kernel(int *__restrict__ a, const int *__restrict__ b, long long n)
{
    const long long i = blockIdx.y, j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j > i) return;
    const size_t at = ((size_t)blockIdx.z * n + i) * n + j;
    a[at] += b[at];
}

unsigned tile_pairs(long long n, int tile)
{
    const long long T = (n + tile - 1) / tile;
    return (unsigned)(T * (T + 1) / 2);
}

}  // namespace

// n <= 65535 and K <= PMDI_KMAX_I are the caller's to check (pmdi_psm_acc_create): every grid below fits
hipError_t pmdi_launch_psm_acc_add(const unsigned char *samples, long long S, int K, long long n, int n_labels, int *counts, hipStream_t stream)
{
    if (S <= 0 || n <= 0 || K <= 0) return hipSuccess;
    if (n_labels >= 1 && n_labels <= 32)
        hipLaunchKernelGGL(psm_acc_mfma_kernel<1>, dim3(tile_pairs(n, 128), (unsigned)K), dim3(256), 0, stream, samples, S, K, n, counts);
    else if (n_labels >= 1 && n_labels <= 64)
        hipLaunchKernelGGL(psm_acc_mfma_kernel<2>, dim3(tile_pairs(n, 128), (unsigned)K), dim3(256), 0, stream, samples, S, K, n, counts);
    else
        hipLaunchKernelGGL(psm_acc_kernel, dim3(tile_pairs(n, 64), (unsigned)K), dim3(256), 0, stream, samples, S, K, n, counts);
    return hipGetLastError();
}

hipError_t pmdi_launch_psm_acc_mirror(int *counts, int K, long long n, hipStream_t stream)
{
    if (n <= 0 || K <= 0) return hipSuccess;
    hipLaunchKernelGGL(psm_acc_mirror_kernel, dim3(tile_pairs(n, 64), (unsigned)K), dim3(256), 0, stream, counts, n);
    return hipGetLastError();
}

hipError_t pmdi_launch_psm_acc_merge(int *a, const int *b, int K, long long n, hipStream_t stream)
{
    if (n <= 0 || K <= 0) return hipSuccess;
    hipLaunchKernelGGL(psm_acc_merge_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)n, (unsigned)K), dim3(256), 0, stream, a, b, n);
    return hipGetLastError();
}
