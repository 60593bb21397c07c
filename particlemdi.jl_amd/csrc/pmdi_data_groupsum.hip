// pmdi_data_groupsum.hip -- sums of a resident data matrix over a grouping of its rows (include/pmdi_hip.h,
// pmdi_data_groupsum_device): out[g][d] = sum_{i in g} v(i, d), v the element itself, its squared deviation from shift[d], its
// z-score bin, or one count into its level.  With the pixel bins of a dendrogram's leaf order as groups this is the data matrix
// of plot_pmdi_data binned to pixels, with cluster labels the sufficient statistics of cluster_add! per cluster and feature.
//
// data_groupsum_kernel: LANES ACROSS THE COLUMNS OF A ROW -- rows are contiguous (x[i * ld + d]), so a wave reads up to 512
//   contiguous bytes of one row per load.  A chunk is at most 32 rows of ONE group (pmdi_psm_blocksum_plan.h).  With D >= 64 a
//   wave owns 64 columns of one chunk (wave = chunk * ceil(D / 64) + column tile); with D < 64, 64 / P chunks share a wave, P
//   the power of two >= D (lane = sub * P + d: chunk = wave * (64 / P) + sub).  Every lane walks its chunk's rows in plan order
//   with ONE accumulator, so the additions of a (chunk, column) happen in exactly the order of the contract; the loads of the
//   rows ahead do not depend on the sum and are issued ahead of it.
//     Float64 results: the lane stores its partial p(c, d) into part[c][d]; data_groupsum_finish_kernel adds them up.
//     Int64 results (exact in any order): the lane adds its partial into out[g][d], zeroed before -- with a plain store when
//     the chunk is its group's only one, with a 64-bit integer atomic otherwise.
//     Levels: one 32-bit integer atomic per element into out[g][d][level - 1], zeroed before.
//   A non-finite element in the z-score mode and a level outside 1..L raise *flag.
// data_groupsum_finish_kernel: one lane per (g, d), lanes across d and on into the next group: out[g][d] = ((0.0 + p(c0, d)) +
//   p(c1, d)) + ... over the chunks of g in plan order (chunks_at[g] .. chunks_at[g + 1]); an empty group stores 0.0.  Every
//   element of out is written.
//
// No LDS, no barrier, no scratch.  No alignment beyond the element's own 8 bytes is assumed: ld may be odd.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pmdi_internal.h"
#include "pmdi_data_groupsum_plan.h"

#pragma clang fp contract(off)      // t = x - shift, v = t * t and the sums are separate IEEE operations (the build passes -ffp-contract=off too)

namespace {

// v(i, d) of the floating-point modes
template <int MODE>
__device__ __forceinline__ double data_value(double x, double shift)
{
    if (MODE == PMDI_DATA_SQDEV_I) {
        const double t = x - shift;
        return t * t;
    }
    return x;
}

// grid: 4 waves per workgroup, wave = blockIdx.x * 4 + (threadIdx.x >> 6); P, cpw, ct: DataGroupsumShape (pmdi_data_groupsum_plan.h).
// T = double: MODE RAW / SQDEV -> part (double), MODE ZBIN -> out (int64).  T = long long: MODE RAW -> out (int64), MODE LEVELS
// -> out (int32 [G][D][L]).
template <typename T, int MODE>
__global__ void __launch_bounds__(256) data_groupsum_kernel(const T *__restrict__ x, int D, long long ld, const int *__restrict__ perm,
                                                            const int *__restrict__ chunk_at, const int *__restrict__ chunk_info,
                                                            int nchunks, int cpw, int P, int ct, const double *__restrict__ shift,
                                                            const double *__restrict__ scale, int L, double *__restrict__ part,
                                                            void *__restrict__ out, int *__restrict__ flag)
{
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    long long c;
    int d;
    data_groupsum_item(P, cpw, ct, wave, lane, c, d);
    if (c >= nchunks || d >= D) return;
    const int r_lo = chunk_at[c], r_hi = chunk_at[c + 1];
    const T *col = x + d;
    constexpr bool F_IN = std::is_same<T, double>::value;
    constexpr bool F_OUT = F_IN && MODE != PMDI_DATA_ZBIN_I;

    if (MODE == PMDI_DATA_LEVELS_I) {
        const int g = chunk_info[c] >> 1;
        int *cell = (int *)out + ((size_t)g * D + d) * (size_t)L;
        bool bad = false;
        for (int r = r_lo; r < r_hi; ++r) {
            const long long lev = (long long)col[(long long)perm[r] * ld];
            if (lev < 1 || lev > L) bad = true;
            else atomicAdd(&cell[lev - 1], 1);
        }
        if (bad) *flag = 1;
        return;
    }

    const double sh = (F_IN && MODE != PMDI_DATA_RAW_I) ? shift[d] : 0.0;
    const double sc = (MODE == PMDI_DATA_ZBIN_I) ? scale[d] : 1.0;
    double facc = 0.0;                                  // the partial starts as 0.0 + v(r0, d)
    long long iacc = 0;
    bool bad = false;
    auto add = [&](T v) {
        if (F_OUT) {
            facc = facc + data_value<MODE>((double)v, sh);
        } else if (MODE == PMDI_DATA_ZBIN_I) {
            const double xv = (double)v;
            double z = floor((xv - sh) / sc);
            z = z > 2.0 ? 2.0 : (z < -2.0 ? -2.0 : z);
            if (!(fabs(xv) <= 1.7976931348623157e308)) {      // NaN or an infinity
                bad = true;
                z = 0.0;
            }
            iacc += (long long)z;
        } else {
            iacc += (long long)v;
        }
    };
    int r = r_lo;
    for (; r + 4 <= r_hi; r += 4) {                    // four loads in flight, added in plan order
        T v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = col[(long long)perm[r + u] * ld];
#pragma unroll
        for (int u = 0; u < 4; ++u) add(v[u]);
    }
    for (; r < r_hi; ++r) add(col[(long long)perm[r] * ld]);
    if (F_OUT) {
        part[(size_t)c * D + d] = facc;
        return;
    }
    if (bad) *flag = 1;
    const int info = chunk_info[c];
    unsigned long long *cell = (unsigned long long *)out + (size_t)(info >> 1) * D + d;
    if (info & 1) {
        if (iacc) atomicAdd(cell, (unsigned long long)iacc);      // several chunks feed this group (out was zeroed)
    } else {
        *cell = (unsigned long long)iacc;
    }
}

// grid: one lane per element of out, g = index / D, d = index % D: neighbouring lanes read neighbouring columns
__global__ void __launch_bounds__(256) data_groupsum_finish_kernel(const double *__restrict__ part, int D, int G, const int *__restrict__ chunks_at,
                                                                   double *__restrict__ out)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)G * D) return;
    const int g = (int)(e / D), d = (int)(e % D);
    const int c_lo = chunks_at[g], c_hi = chunks_at[g + 1];
    double acc = 0.0;
    const double *p = part + (size_t)c_lo * D + d;
    int c = c_lo;
    // a group of a few labels has hundreds of chunks and this lane walks them alone: 16 loads in flight, then 4, added in plan order
    for (; c + 16 <= c_hi; c += 16, p += (size_t)16 * D) {
        double a[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) a[u] = p[(size_t)u * D];
#pragma unroll
        for (int u = 0; u < 16; ++u) acc = acc + a[u];
    }
    for (; c + 4 <= c_hi; c += 4, p += (size_t)4 * D) {
        double a[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = p[(size_t)u * D];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = acc + a[u];
    }
    for (; c < c_hi; ++c, p += D) acc = acc + p[0];
    out[(size_t)g * D + d] = acc;
}

template <typename T, int MODE>
void launch_chunks(const T *x, int D, long long ld, const int *perm, const int *chunk_at, const int *chunk_info, int nchunks,
                   const double *shift, const double *scale, int L, double *part, void *out, int *flag, hipStream_t stream)
{
    const DataGroupsumShape s = data_groupsum_shape(D, nchunks);
    hipLaunchKernelGGL((data_groupsum_kernel<T, MODE>), dim3((unsigned)((s.waves + 3) / 4)), dim3(256), 0, stream, x, D, ld, perm, chunk_at,
                       chunk_info, nchunks, s.cpw, s.P, s.ct, shift, scale, L, part, out, flag);
}

}  // namespace

// The tables of PsmBlocksumPlan on the device (chunks_at [G + 1]: the first chunk of every group); shift, scale [D] or null as
// the mode needs; part [nchunks][D] doubles for a Float64 result, else null; flag zeroed by the caller.  out: [G][D] doubles or
// int64, or [G][D][L] int32, every element written.  Everything pmdi_data_groupsum_device checks is the caller's to check.
hipError_t pmdi_launch_data_groupsum(int is_float, const void *x, int D, long long ld, int G, int mode, const int *perm, const int *chunk_at,
                                     const int *chunk_info, int nchunks, const int *chunks_at, const double *shift, const double *scale,
                                     int L, double *part, void *out, int *flag, hipStream_t stream)
{
    const bool f_out = is_float && (mode == PMDI_DATA_RAW_I || mode == PMDI_DATA_SQDEV_I);
    if (!f_out) {
        const size_t bytes = mode == PMDI_DATA_LEVELS_I ? (size_t)G * D * (size_t)L * 4 : (size_t)G * D * 8;
        const hipError_t e = hipMemsetAsync(out, 0, bytes, stream);
        if (e != hipSuccess) return e;
    }
    const double *xf = (const double *)x;
    const long long *xi = (const long long *)x;
    if (is_float && mode == PMDI_DATA_RAW_I)
        launch_chunks<double, PMDI_DATA_RAW_I>(xf, D, ld, perm, chunk_at, chunk_info, nchunks, shift, scale, L, part, out, flag, stream);
    else if (is_float && mode == PMDI_DATA_SQDEV_I)
        launch_chunks<double, PMDI_DATA_SQDEV_I>(xf, D, ld, perm, chunk_at, chunk_info, nchunks, shift, scale, L, part, out, flag, stream);
    else if (is_float && mode == PMDI_DATA_ZBIN_I)
        launch_chunks<double, PMDI_DATA_ZBIN_I>(xf, D, ld, perm, chunk_at, chunk_info, nchunks, shift, scale, L, part, out, flag, stream);
    else if (!is_float && mode == PMDI_DATA_RAW_I)
        launch_chunks<long long, PMDI_DATA_RAW_I>(xi, D, ld, perm, chunk_at, chunk_info, nchunks, shift, scale, L, part, out, flag, stream);
    else if (!is_float && mode == PMDI_DATA_LEVELS_I)
        launch_chunks<long long, PMDI_DATA_LEVELS_I>(xi, D, ld, perm, chunk_at, chunk_info, nchunks, shift, scale, L, part, out, flag, stream);
    else
        return hipErrorInvalidValue;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !f_out) return e;
    hipLaunchKernelGGL(data_groupsum_finish_kernel, dim3((unsigned)(((long long)G * D + 255) / 256)), dim3(256), 0, stream, part, D, G,
                       chunks_at, (double *)out);
    return hipGetLastError();
}
