// pmdi_partdist.hip -- partition distances between candidate clusterings and sampled clusterings (include/pmdi_hip.h,
// pmdi_partition_rows_device, pmdi_partition_distance_device): what Binder's loss, the variation of information and the adjusted
// Rand index between two clusterings need, as exact integers.
//   partdist_rows_kernel      one wavefront per label row: the labels (int32 or bytes, rows `ld` elements apart) once, as bytes
//                             [np] with MX_PAD behind n; the label histogram b_h, sum_h C(b_h, 2), sum_h b_h L(b_h) and the number
//                             of occupied labels
//   partdist_kernel           the hot path.  One workgroup per draw row: its bytes staged in LDS, one wavefront per candidate;
//                             the contingency table n_gh = #{i : c_i = g, s_i = h} is a product of one-hot int8 matrices with
//                             the observations as the inner dimension (v_mfma_i32_32x32x32_i8) and lives in the accumulators
//                             only: both = sum_gh C(n_gh, 2), jl = sum_gh n_gh L(n_gh)
// L is the fixed-point logarithm of pmdi_fixlog.h (the table of pmdi_vi_log2_table.h, here in LDS).  Every output word
// is owned by one wave and every sum is an integer: the results are bit-defined.
#include <hip/hip_runtime.h>

#include "pmdi_fixlog.h"            // L in 32-bit steps and v L(v)
#include "pmdi_internal.h"
#include "pmdi_onehot.h"            // the fragment types, MX_PAD, mx_wave_sync, mx_wave_sum, mx_onehot

namespace {

#define PD_TABLE PMDI_FIXLOG_TABLE
#define PD_CHUNK 1024   // candidate label bytes a wave stages per round: 16 per lane

__device__ const int pd_table[PD_TABLE] = {
#include "pmdi_vi_log2_table.h"
};

// Row `row` of s (row r at s + r ld, n labels of unit stride) into bytes out [rows][np] (np = n rounded up to 32; the bytes
// behind n are MX_PAD), one wavefront per row, 4 rows per workgroup; a lane packs four consecutive labels into one aligned
// dword.  The histogram of the row is built in the wave's own 256 LDS bins.  A label >= G (a negative one is a large one) sets
// *err, goes out as MX_PAD and is counted nowhere: nothing is indexed by it.
template <typename T>
__global__ void __launch_bounds__(256) partdist_rows_kernel(const T *__restrict__ s, long long n_rows, long long n, long long ld, int np, int G,
                                                            unsigned char *__restrict__ out, long long *__restrict__ pairs,
                                                            long long *__restrict__ hl, int *__restrict__ nclust, int *__restrict__ err)
{
    __shared__ int hist[4][256];
    __shared__ int tab[PD_TABLE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = threadIdx.x; k < PD_TABLE; k += 256) tab[k] = pd_table[k];
    int *h = hist[wave];
    for (int i = lane; i < 256; i += 64) h[i] = 0;
    __syncthreads();                                         // (before any wave leaves: the only workgroup barrier)
    const long long row = (long long)blockIdx.x * 4 + wave;
    if (row >= n_rows) return;                               // (the same in every lane of a wave)
    const T *p = s + row * ld;
    unsigned *o = (unsigned *)(out + row * np);
    unsigned bad = 0u;
    const int nd = np >> 2;
#pragma unroll 4
    for (int j = lane; j < nd; j += 64) {
        unsigned u[4], w = 0u;
#pragma unroll
        for (int b = 0; b < 4; ++b) {                        // every address is clamped into the row and the guard selects
            const long long i = 4ll * j + b;                 // afterwards: no load sits under a branch
            u[b] = (unsigned)p[i < n ? i : n - 1];           // a negative label is a large one
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const bool in_row = 4ll * j + b < n, ok = in_row && u[b] < (unsigned)G;
            if (ok) atomicAdd(&h[u[b]], 1);
            bad |= (in_row && !ok) ? 1u : 0u;
            w |= (ok ? u[b] : MX_PAD) << (8 * b);
        }
        o[j] = w;
    }
    mx_wave_sync();
    unsigned long long pr = 0ull, lg = 0ull, occupied = 0ull;
    for (int a = lane; a < G; a += 64) {
        const unsigned c = (unsigned)h[a];                   // <= 65535: c (c - 1) / 2 < 2^31
        pr += (unsigned long long)((c * (c - 1u)) >> 1);     // (c = 0: the product is 0 whatever c - 1 wrapped to)
        lg += pmdi_fixlog_vL32(c, tab);
        occupied += c ? 1ull : 0ull;
    }
    pr = mx_wave_sum(pr);
    lg = mx_wave_sum(lg);
    occupied = mx_wave_sum(occupied);
    bad |= (unsigned)__shfl_xor((int)bad, 32); bad |= (unsigned)__shfl_xor((int)bad, 16); bad |= (unsigned)__shfl_xor((int)bad, 8);
    bad |= (unsigned)__shfl_xor((int)bad, 4); bad |= (unsigned)__shfl_xor((int)bad, 2); bad |= (unsigned)__shfl_xor((int)bad, 1);
    if (lane == 0) {
        pairs[row] = (long long)pr;
        hl[row] = (long long)lg;
        nclust[row] = (int)occupied;
        if (bad) *err = 1;
    }
}

// both[b R + r] = sum_gh n_gh (n_gh - 1) / 2 and jl[b R + r] = sum_gh n_gh L(n_gh), n_gh = observations with label g in candidate
// b and label h in draw r.  Workgroup = draw row r; its bytes [np] are staged once, the table of L behind them; wave w takes
// the candidates w, w + 4, ... and walks the candidate's row in rounds of PD_CHUNK bytes through its own staging buffer.  One
// MFMA covers 32 observations x (32 x 32) labels: lane (q = lane & 31, h = lane >> 5) holds [c_i == label q] for the 16
// observations i0 + 16 h .. + 15 as the A fragment and [s_i == label q] as the B fragment; the hardware pairs byte j of half h on
// both sides, so the sum over the inner dimension runs over the same observation.  NC, ND = 32-label tiles per side of one pass
// (1: at most 32 labels on that side, else 2); the passes run over the ceil(Gc / (32 NC)) x ceil(Gd / (32 ND)) pairs of label
// blocks -- one pass up to 64 labels a side, 64-label blocks beyond.  Only sums over the table are wanted, so the C/D layout
// does not enter.  After the one workgroup barrier behind the staging the waves run apart: a wave's staging buffer is its own
// and needs wave-level ordering only.  The padding bytes (MX_PAD) match no label on either side: Gc, Gd <= 255.
template <int NC, int ND>
__global__ void __launch_bounds__(256) partdist_kernel(const unsigned char *__restrict__ cand, const unsigned char *__restrict__ draws, int np,
                                                       int Gc, int Gd, long long B, long long R, long long *__restrict__ both,
                                                       long long *__restrict__ jl)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char pd_lds[];
    mx_v4u *cur = (mx_v4u *)pd_lds;                          // [np / 16]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    mx_v4u *stage = (mx_v4u *)(pd_lds + np) + wave * (PD_CHUNK / 16);      // [64], this wave's
    int *tab = (int *)(pd_lds + np + 4 * PD_CHUNK);          // [PD_TABLE]
    const int q = lane & 31, h = lane >> 5;
    const long long row = blockIdx.x;
    {
        const mx_v4u *src = (const mx_v4u *)(draws + row * np);
        for (int i = tid; i < (np >> 4); i += 256) cur[i] = src[i];
        for (int k = tid; k < PD_TABLE; k += 256) tab[k] = pd_table[k];
    }
    __syncthreads();
    const int nbc = (Gc + 32 * NC - 1) / (32 * NC), nbd = (Gd + 32 * ND - 1) / (32 * ND);
    for (long long b = wave; b < B; b += 4) {
        const mx_v4u *cp = (const mx_v4u *)(cand + b * np);
        unsigned long long t_both = 0ull, t_jl = 0ull;
        for (int bc = 0; bc < nbc; ++bc)
            for (int bd = 0; bd < nbd; ++bd) {
                unsigned rep_c[NC], one_c[NC], rep_d[ND], one_d[ND];
#pragma unroll
                for (int i = 0; i < NC; ++i) {
                    const unsigned l = (unsigned)(32 * NC * bc + 32 * i + q);
                    rep_c[i] = l * 0x01010101u; one_c[i] = l < (unsigned)Gc ? 0x01010101u : 0u;
                }
#pragma unroll
                for (int j = 0; j < ND; ++j) {
                    const unsigned l = (unsigned)(32 * ND * bd + 32 * j + q);
                    rep_d[j] = l * 0x01010101u; one_d[j] = l < (unsigned)Gd ? 0x01010101u : 0u;
                }
                mx_v16i acc[NC][ND];
#pragma unroll
                for (int i = 0; i < NC; ++i)
#pragma unroll
                    for (int j = 0; j < ND; ++j)
#pragma unroll
                        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0;
                for (int c0 = 0; c0 < np; c0 += PD_CHUNK) {
                    const int left = np - c0;                // a multiple of 32
                    mx_v4u v = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
                    if (16 * lane < left) v = cp[(c0 >> 4) + lane];
                    mx_wave_sync();                          // the steps of the last round have read the buffer
                    stage[lane] = v;
                    mx_wave_sync();
                    const int steps = left < PD_CHUNK ? left >> 5 : PD_CHUNK / 32;
                    for (int st = 0; st < steps; ++st) {
                        const mx_v4u c16 = stage[2 * st + h], d16 = cur[(c0 >> 4) + 2 * st + h];
                        mx_v4i fc[NC], fd[ND];
#pragma unroll
                        for (int i = 0; i < NC; ++i) fc[i] = mx_onehot(c16, rep_c[i], one_c[i]);
#pragma unroll
                        for (int j = 0; j < ND; ++j) fd[j] = mx_onehot(d16, rep_d[j], one_d[j]);
#pragma unroll
                        for (int i = 0; i < NC; ++i)
#pragma unroll
                            for (int j = 0; j < ND; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fc[i], fd[j], acc[i][j], 0, 0, 0);
                    }
                }
#pragma unroll
                for (int i = 0; i < NC; ++i)
#pragma unroll
                    for (int j = 0; j < ND; ++j)
#pragma unroll
                        for (int e = 0; e < 16; ++e) {
                            const unsigned c = (unsigned)acc[i][j][e];       // <= 65535: c (c - 1) / 2 < 2^31, c L(c) < 2^50
                            t_both += (unsigned long long)((c * (c - 1u)) >> 1);
                            t_jl += pmdi_fixlog_vL32(c, tab);
                        }
            }
        t_both = mx_wave_sum(t_both);
        t_jl = mx_wave_sum(t_jl);
        if (lane == 0) { both[b * R + row] = (long long)t_both; jl[b * R + row] = (long long)t_jl; }
    }
}

template <int NC, int ND>
hipError_t launch_partdist(const unsigned char *cand, const unsigned char *draws, int np, int Gc, int Gd, long long B, long long R,
                           long long *both, long long *jl, hipStream_t stream)
{
    const size_t lds = (size_t)np + 4 * PD_CHUNK + PD_TABLE * sizeof(int);
    auto fn = partdist_kernel<NC, ND>;
    if (lds > 65536) {                                       // (beyond the default limit of dynamic LDS: n > 53 216 only)
        hipError_t e = hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(fn, dim3((unsigned)R), dim3(256), lds, stream, cand, draws, np, Gc, Gd, B, R, both, jl);
    return hipGetLastError();
}

}  // namespace

// 1 <= R <= INT32_MAX, 1 <= n <= 65535, ld >= n, 1 <= G <= 255 are the caller's to check (pmdi_partition_rows_device).
// bytes [R][np], np = n rounded up to 32; pairs, hl [R] int64; nclust [R] int32; err [1], zero before the launch.
hipError_t pmdi_launch_partition_rows(const void *labels, int is_bytes, long long R, long long n, long long ld, int G, unsigned char *bytes,
                                      long long *pairs, long long *hl, int *nclust, int *err, hipStream_t stream)
{
    const int np = (int)((n + 31) / 32 * 32);
    const dim3 grid((unsigned)((R + 3) / 4));
    if (is_bytes)
        hipLaunchKernelGGL(partdist_rows_kernel<unsigned char>, grid, dim3(256), 0, stream, (const unsigned char *)labels, R, n, ld, np, G, bytes,
                           pairs, hl, nclust, err);
    else
        hipLaunchKernelGGL(partdist_rows_kernel<int>, grid, dim3(256), 0, stream, (const int *)labels, R, n, ld, np, G, bytes, pairs, hl, nclust, err);
    return hipGetLastError();
}

// cand [B][np], draws [R][np] as pmdi_launch_partition_rows writes them; both, jl [B][R].  1 <= B, 1 <= R <= INT32_MAX,
// 1 <= n <= 65535, 1 <= Gc, Gd <= 255 are the caller's to check (pmdi_partition_distance_device).
hipError_t pmdi_launch_partition_distance(const unsigned char *cand, long long B, int Gc, const unsigned char *draws, long long R, int Gd,
                                          long long n, long long *both, long long *jl, hipStream_t stream)
{
    const int np = (int)((n + 31) / 32 * 32);
    return Gc <= 32 ? (Gd <= 32 ? launch_partdist<1, 1>(cand, draws, np, Gc, Gd, B, R, both, jl, stream)
                                : launch_partdist<1, 2>(cand, draws, np, Gc, Gd, B, R, both, jl, stream))
                    : (Gd <= 32 ? launch_partdist<2, 1>(cand, draws, np, Gc, Gd, B, R, both, jl, stream)
                                : launch_partdist<2, 2>(cand, draws, np, Gc, Gd, B, R, both, jl, stream));
}
