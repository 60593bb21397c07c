// pmdi_psm_acc.hip -- the streaming PSM accumulator (include/pmdi_hip.h, pmdi_psm_acc_*): the accumulating counterparts of
// psm_count_kernel / psm_count_mfma_kernel (pmdi_kernels.hip).  Each pair of kernels runs one body (pmdi_psm_device.h:
// psm_count_body, psm_count_mfma_body); the kernels here differ from the one-shot ones in two ways:
//   * counts += tile.  Every (dataset, tile) belongs to exactly one workgroup of a launch and the launches of one
//     accumulator are ordered on one stream, so this is a plain read-modify-write: no atomics.
//   * only the tiles with block-row >= block-column are computed (the counts are symmetric); grid.x walks the
//     T (T + 1) / 2 lower tile pairs, diagonal tiles are computed whole.  The strict upper triangle is filled once, by
//     psm_acc_mirror_kernel, when the counts are asked for.
// Integer compares, int8 products and int32 sums only: exact by construction.
#include <hip/hip_runtime.h>

#include "pmdi_internal.h"
#include "pmdi_psm_device.h"

namespace {

// grid: x = tile pair (64-wide tiles), y = dataset
__global__ void __launch_bounds__(256) psm_acc_kernel(const unsigned char *__restrict__ samples, long long S, int K, long long n,
                                                      int *__restrict__ counts)
{
    int bi, bj;
    psm_tile_pair(blockIdx.x, bi, bj);
    psm_count_body<true>(PsmStageLabel{(int)blockIdx.y}, samples, S, K, n, blockIdx.y, (long long)bi * 64, (long long)bj * 64, n, n, 0, counts);
}

// grid: x = tile pair (128-wide tiles), y = dataset.
// 4 waves per SIMD asked for: the read half of counts += tile (64 loads and their addresses per lane) would otherwise set the
// kernel's register count (106 VGPRs + 64 AGPRs, 2 waves per SIMD) where the sample loop lives on half of that.
template <int NKB>
__global__ void __launch_bounds__(256, 4) psm_acc_mfma_kernel(const unsigned char *__restrict__ samples, long long S, int K, long long n,
                                                           int *__restrict__ counts)
{
    int bi, bj;
    psm_tile_pair(blockIdx.x, bi, bj);
    psm_count_mfma_body<NKB, true>(PsmStageLabel{(int)blockIdx.y}, samples, S, K, n, blockIdx.y, (long long)bi * 128, (long long)bj * 128, n, n, 0, counts);
}

// counts[k][j][i] = counts[k][i][j] for i > j: a 64 x 64 tile of the lower triangle is read row-wise, transposed through LDS
// (65-int rows: no bank conflicts) and written row-wise into its mirror image.  A diagonal tile writes its own strict upper part.
__global__ void __launch_bounds__(256) psm_acc_mirror_kernel(int *__restrict__ counts, long long n)
{
    __shared__ int tile[64][65];
    const int k = blockIdx.y;
    int bi, bj;
    psm_tile_pair(blockIdx.x, bi, bj);
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

}  // namespace

// n <= 65535 and K <= PMDI_KMAX_I are the caller's to check (pmdi_psm_acc_create): every grid below fits
hipError_t pmdi_launch_psm_acc_add(const unsigned char *samples, long long S, int K, long long n, int n_labels, int *counts, hipStream_t stream)
{
    if (S <= 0 || n <= 0 || K <= 0) return hipSuccess;
    if (n_labels >= 1 && n_labels <= 32)
        hipLaunchKernelGGL(psm_acc_mfma_kernel<1>, dim3(psm_tile_pairs(n, 128), (unsigned)K), dim3(256), 0, stream, samples, S, K, n, counts);
    else if (n_labels >= 1 && n_labels <= 64)
        hipLaunchKernelGGL(psm_acc_mfma_kernel<2>, dim3(psm_tile_pairs(n, 128), (unsigned)K), dim3(256), 0, stream, samples, S, K, n, counts);
    else
        hipLaunchKernelGGL(psm_acc_kernel, dim3(psm_tile_pairs(n, 64), (unsigned)K), dim3(256), 0, stream, samples, S, K, n, counts);
    return hipGetLastError();
}

hipError_t pmdi_launch_psm_acc_mirror(int *counts, int K, long long n, hipStream_t stream)
{
    if (n <= 0 || K <= 0) return hipSuccess;
    hipLaunchKernelGGL(psm_acc_mirror_kernel, dim3(psm_tile_pairs(n, 64), (unsigned)K), dim3(256), 0, stream, counts, n);
    return hipGetLastError();
}

hipError_t pmdi_launch_psm_acc_merge(int *a, const int *b, int K, long long n, hipStream_t stream)
{
    if (n <= 0 || K <= 0) return hipSuccess;
    hipLaunchKernelGGL(psm_acc_merge_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)n, (unsigned)K), dim3(256), 0, stream, a, b, n);
    return hipGetLastError();
}
