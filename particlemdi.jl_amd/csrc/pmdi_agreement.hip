// pmdi_agreement.hip -- the streaming agreement accumulator (include/pmdi_hip.h, pmdi_agreement_*): how alike two datasets
// cluster the observations, and how alike a dataset's clustering and a labelling known in advance are, taken from every
// retained iteration of every chain on the device.  A comparison q has two sides x (a dataset's labels) and y (another dataset's
// labels, or the classes of a reference labelling with MX_PAD where the class is unknown).  One add is 3 + R launches on the
// accumulator's stream:
//   agreement_rows_kernel         one wavefront per (chain, dataset) row: the int32 labels once, as bytes [np] with MX_PAD for a
//                                 label outside 0..N-1 and behind n
//   agreement_contingency_kernel  the hot path.  One workgroup per chain, one wavefront per comparison: the contingency table
//                                 n_ab = #{i : x_i = a, y_i = b} is a product of one-hot int8 matrices with the observations as
//                                 the inner dimension (v_mfma_i32_32x32x32_i8) and lives in the accumulators only.  An
//                                 observation with MX_PAD on either side matches no one-hot row and is in no cell, so the
//                                 marginals are taken from the table itself: they are its row and column sums by construction,
//                                 whatever is unknown or out of range.  One launch for the dataset pairs, one per reference (its
//                                 number of classes picks the tiles of the y side).
//   agreement_finish_kernel       one lane per (chain, comparison): the sums and the histogram; one lane per comparison of the
//                                 last workgroup: the trace row, the chains staged through LDS and added in chain order
// L is the fixed-point logarithm of pmdi_fixlog.h (the table of pmdi_vi_log2_table.h).  Every word of the state is owned by one
// lane of a launch or is an integer atomic, and the launches are ordered on one stream: the state is bit-defined by the order
// of the adds.
#include <hip/hip_runtime.h>

#include "pmdi_fixlog.h"            // L in 32-bit steps and v L(v)
#include "pmdi_internal.h"
#include "pmdi_onehot.h"            // the fragment types, MX_PAD, mx_wave_sync, mx_wave_sum, mx_onehot

#pragma clang fp contract(off)      // the sums are defined with separate multiplies and adds (the build passes -ffp-contract=off too)

namespace {

#define AG_TABLE PMDI_FIXLOG_TABLE
#define AG_CHUNK 1024   // label bytes of one side a wave stages per round: 16 per lane
#define AG_STAGE 2048   // doubles of the finish kernel's stage: at least 22 chains per round (Q <= 92)

__device__ const int ag_table[AG_TABLE] = {
#include "pmdi_vi_log2_table.h"
};

// Row `row` = chain * K + dataset of s [rows][n] into bytes out [rows][np] (np = n rounded up to 32; the bytes behind n are
// MX_PAD), one wavefront per row, 4 rows per workgroup (mx_label_row).  A label outside 0..N-1 goes out as MX_PAD and sets *err.
__global__ void __launch_bounds__(256) agreement_rows_kernel(const int *__restrict__ s, long long n_rows, long long n, int np, int N,
                                                             unsigned char *__restrict__ out, int *__restrict__ err)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row = (long long)blockIdx.x * 4 + wave;
    if (row >= n_rows) return;                               // (the same in every lane of a wave; no barrier below)
    const bool bad = mx_label_row(s + row * n, n, np, N, (unsigned *)(out + row * np), lane);
    if (lane == 0 && bad) *err = 1;
}

// last[chain][q0 + i][0..6] = both, jl, px, py, hx, hy, n_q of comparison q0 + i, i = 0..nq-1, of every chain.  yref == null:
// the comparisons are the dataset pairs (a < b) in the order of Phi, x = row a and y = row b of the chain's bytes, nq = G;
// else x = row i and y = yref [np], the class bytes of one reference, nq = K.  Workgroup = chain; wave w takes the comparisons
// w, w + 4, ... and walks both sides in rounds of AG_CHUNK bytes through its own two staging buffers, so the LDS does not grow
// with n.  One MFMA covers 32 observations x (32 x 32) labels: lane (r = lane & 31, h = lane >> 5) holds [x_i == label r] for
// the 16 observations i0 + 16 h .. + 15 as the A fragment and [y_i == label r] as the B fragment; the hardware pairs byte j of
// half h on both sides, so the sum over the inner dimension runs over the same observation.  NX, NY = 32-label tiles per side
// of one pass (1: at most 32 labels on that side, else 2), chosen separately: a reference may have more classes than N, or
// fewer; the passes run over the ceil(Gx / (32 NX)) x ceil(Gy / (32 NY)) pairs of label blocks.
// Of the C/D layout only this enters: an entry's column is lane & 31, and its row depends on (register, h) alone and differs
// between any two of them.  So the sum of a lane's 16 registers plus that of lane ^ 32 is a column sum of the tile, and the
// sum of one register over the 32 lanes of a half is a row sum.  Row sums are carried in registers over the inner loop of y
// blocks, column sums in the wave's own 256 LDS words over the outer loop of x blocks (only this wave touches them: plain
// adds, wave-level ordering).
template <int NX, int NY>
__global__ void __launch_bounds__(256) agreement_contingency_kernel(const unsigned char *__restrict__ bytes, const unsigned char *__restrict__ yref,
                                                                    int K, int np, int Gx, int Gy, int q0, int nq, int Q,
                                                                    long long *__restrict__ last)
{
    __shared__ __attribute__((aligned(16))) mx_v4u stage[4][2][AG_CHUNK / 16];
    __shared__ int colsum[4][256];
    __shared__ int tab[AG_TABLE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const long long chain = blockIdx.x;
    for (int k = tid; k < AG_TABLE; k += 256) tab[k] = ag_table[k];
    for (int i = lane; i < 256; i += 64) colsum[wave][i] = 0;
    __syncthreads();                                         // (the only workgroup barrier; the waves run apart behind it)
    mx_v4u *sx = stage[wave][0], *sy = stage[wave][1];
    int *cs = colsum[wave];
    const int nbx = (Gx + 32 * NX - 1) / (32 * NX), nby = (Gy + 32 * NY - 1) / (32 * NY);
    for (int qi = wave; qi < nq; qi += 4) {
        int xa = qi, yb = 0;
        if (!yref) {                                         // pair number qi in the order (0,1), (0,2), ..., (K-2,K-1)
            int left = qi;
            xa = 0;
            while (left >= K - 1 - xa) { left -= K - 1 - xa; ++xa; }
            yb = xa + 1 + left;
        }
        const mx_v4u *xp = (const mx_v4u *)(bytes + (chain * K + xa) * np);
        const mx_v4u *yp = (const mx_v4u *)(yref ? yref : bytes + (chain * K + yb) * np);
        unsigned long long t_both = 0ull, t_jl = 0ull, t_px = 0ull, t_hx = 0ull, t_n = 0ull;
        for (int bx = 0; bx < nbx; ++bx) {
            unsigned rep_x[NX], one_x[NX];
#pragma unroll
            for (int i = 0; i < NX; ++i) {
                const unsigned l = (unsigned)(32 * NX * bx + 32 * i + r);
                rep_x[i] = l * 0x01010101u; one_x[i] = l < (unsigned)Gx ? 0x01010101u : 0u;
            }
            int rowacc[NX][16];
#pragma unroll
            for (int i = 0; i < NX; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) rowacc[i][e] = 0;
            for (int by = 0; by < nby; ++by) {
                unsigned rep_y[NY], one_y[NY];
#pragma unroll
                for (int j = 0; j < NY; ++j) {
                    const unsigned l = (unsigned)(32 * NY * by + 32 * j + r);
                    rep_y[j] = l * 0x01010101u; one_y[j] = l < (unsigned)Gy ? 0x01010101u : 0u;
                }
                mx_v16i acc[NX][NY];
#pragma unroll
                for (int i = 0; i < NX; ++i)
#pragma unroll
                    for (int j = 0; j < NY; ++j)
#pragma unroll
                        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0;
                for (int c0 = 0; c0 < np; c0 += AG_CHUNK) {
                    const int left = np - c0;                // a multiple of 32
                    mx_v4u vx = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, vy = vx;
                    if (16 * lane < left) { vx = xp[(c0 >> 4) + lane]; vy = yp[(c0 >> 4) + lane]; }
                    mx_wave_sync();                          // the steps of the last round have read the buffers
                    sx[lane] = vx;
                    sy[lane] = vy;
                    mx_wave_sync();
                    const int steps = left < AG_CHUNK ? left >> 5 : AG_CHUNK / 32;
                    for (int st = 0; st < steps; ++st) {
                        const mx_v4u x16 = sx[2 * st + h], y16 = sy[2 * st + h];
                        mx_v4i fx[NX], fy[NY];
#pragma unroll
                        for (int i = 0; i < NX; ++i) fx[i] = mx_onehot(x16, rep_x[i], one_x[i]);
#pragma unroll
                        for (int j = 0; j < NY; ++j) fy[j] = mx_onehot(y16, rep_y[j], one_y[j]);
#pragma unroll
                        for (int i = 0; i < NX; ++i)
#pragma unroll
                            for (int j = 0; j < NY; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fx[i], fy[j], acc[i][j], 0, 0, 0);
                    }
                }
                int col[NY];
#pragma unroll
                for (int j = 0; j < NY; ++j) col[j] = 0;
#pragma unroll
                for (int i = 0; i < NX; ++i)
#pragma unroll
                    for (int j = 0; j < NY; ++j)
#pragma unroll
                        for (int e = 0; e < 16; ++e) {
                            const unsigned c = (unsigned)acc[i][j][e];       // <= 65535: c (c - 1) / 2 < 2^31, c L(c) < 2^50
                            t_both += (unsigned long long)((c * (c - 1u)) >> 1);
                            t_jl += pmdi_fixlog_vL32(c, tab);
                            rowacc[i][e] += (int)c;
                            col[j] += (int)c;
                        }
#pragma unroll
                for (int j = 0; j < NY; ++j) {
                    const int both_halves = col[j] + __shfl_xor(col[j], 32);
                    if (h == 0) cs[32 * NY * by + 32 * j + r] += both_halves;      // (32 NY by + 32 j + r < 32 NY nby <= 256)
                }
            }
#pragma unroll
            for (int i = 0; i < NX; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    int v = rowacc[i][e];
                    v += __shfl_xor(v, 16); v += __shfl_xor(v, 8); v += __shfl_xor(v, 4); v += __shfl_xor(v, 2); v += __shfl_xor(v, 1);
                    const unsigned c = r == 0 ? (unsigned)v : 0u;            // one lane per half counts the row
                    t_px += (unsigned long long)((c * (c - 1u)) >> 1);
                    t_hx += pmdi_fixlog_vL32(c, tab);
                    t_n += c;
                }
        }
        mx_wave_sync();                                      // the column sums of every lane are in cs
        unsigned long long t_py = 0ull, t_hy = 0ull;
        for (int b = lane; b < 256; b += 64) {
            const unsigned c = (unsigned)cs[b];
            cs[b] = 0;                                       // (for this wave's next comparison)
            t_py += (unsigned long long)((c * (c - 1u)) >> 1);
            t_hy += pmdi_fixlog_vL32(c, tab);
        }
        t_both = mx_wave_sum(t_both); t_jl = mx_wave_sum(t_jl);
        t_px = mx_wave_sum(t_px); t_py = mx_wave_sum(t_py);
        t_hx = mx_wave_sum(t_hx); t_hy = mx_wave_sum(t_hy);
        t_n = mx_wave_sum(t_n);
        if (lane == 0) {
            long long *o = last + (chain * Q + q0 + qi) * 7;
            o[0] = (long long)t_both; o[1] = (long long)t_jl; o[2] = (long long)t_px; o[3] = (long long)t_py;
            o[4] = (long long)t_hx; o[5] = (long long)t_hy; o[6] = (long long)t_n;
        }
        mx_wave_sync();
    }
}

// The adjusted Rand index of one comparison from its integers, separate IEEE operations in mixing_finish_kernel's order
__device__ __forceinline__ double ag_ari(long long both, long long px, long long py, long long T2)
{
    double ari = 1.0;
    if (T2 != 0) {
        const double e = (double)px * (double)py / (double)T2;
        const double m = ((double)px + (double)py) / 2.0;
        const double den = m - e;
        ari = (den == 0.0) ? 1.0 : ((double)both - e) / den;
    }
    return ari;
}

// Blocks 0 .. blocks_items - 1: one lane per (chain, comparison) -- the sums and the histogram of this add.  The block behind
// them (launched only while the trace has rows left): the trace row.  The chains go through LDS in rounds of AG_STAGE / Q: the
// whole workgroup forms the round's adjusted Rand indices (the same function of the same integers: the same bits), then lane
// q adds its column in chain order.
__global__ void __launch_bounds__(256) agreement_finish_kernel(AgreementArgs a, unsigned blocks_items, double *__restrict__ trace_row)
{
    __shared__ double stage[AG_STAGE];
    const int Q = a.Q;
    const long long total = (long long)a.C * Q;
    if (blockIdx.x < blocks_items) {
        for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)blocks_items * 256) {
            const int q = (int)(idx % Q);
            const long long *v = a.last + idx * 7;
            const long long both = v[0], jl = v[1], px = v[2], py = v[3], hx = v[4], hy = v[5], nq = v[6];
            const long long T2 = nq * (nq - 1) / 2;
            a.rand_num[idx] += T2 + 2 * both - px - py;
            const double ari = ag_ari(both, px, py, T2);
            a.ari_sum[idx] = a.ari_sum[idx] + ari;
            a.ari_sq[idx] = a.ari_sq[idx] + ari * ari;
            a.vi_sum[idx] += hx + hy - 2 * jl;
            a.mi_sum[idx] += pmdi_fixlog_sL((int)nq, ag_table) - hx - hy + jl;
            int bin = (int)floor((ari + 1.0) * 128.0);
            bin = bin < 0 ? 0 : bin > 255 ? 255 : bin;
            atomicAdd((unsigned long long *)a.ari_hist + (q * 256 + bin), 1ull);
        }
        return;
    }
    const int chunk = AG_STAGE / Q;
    double acc = 0.0;
    for (long long c0 = 0; c0 < a.C; c0 += chunk) {
        const int nc = (a.C - c0 < chunk) ? (int)(a.C - c0) : chunk;
        for (int i = threadIdx.x; i < nc * Q; i += 256) {
            const long long *v = a.last + (c0 * Q + i) * 7;
            const long long nq = v[6];
            stage[i] = ag_ari(v[0], v[2], v[3], nq * (nq - 1) / 2);
        }
        __syncthreads();
        if ((int)threadIdx.x < Q)
            for (int c = 0; c < nc; ++c) acc = acc + stage[c * Q + threadIdx.x];
        __syncthreads();
    }
    if ((int)threadIdx.x < Q) trace_row[threadIdx.x] = acc;
}

template <int NX, int NY>
hipError_t launch_contingency(const AgreementArgs &a, const unsigned char *yref, int Gy, int q0, int nq, hipStream_t stream)
{
    hipLaunchKernelGGL((agreement_contingency_kernel<NX, NY>), dim3((unsigned)a.C), dim3(256), 0, stream, (const unsigned char *)a.bytes, yref,
                       a.K, a.np, a.N, Gy, q0, nq, a.Q, a.last);
    return hipGetLastError();
}

hipError_t contingency(const AgreementArgs &a, const unsigned char *yref, int Gy, int q0, int nq, hipStream_t stream)
{
    return a.N <= 32 ? (Gy <= 32 ? launch_contingency<1, 1>(a, yref, Gy, q0, nq, stream) : launch_contingency<1, 2>(a, yref, Gy, q0, nq, stream))
                     : (Gy <= 32 ? launch_contingency<2, 1>(a, yref, Gy, q0, nq, stream) : launch_contingency<2, 2>(a, yref, Gy, q0, nq, stream));
}

}  // namespace

// 1 <= C, 1 <= K <= PMDI_KMAX_I, 2 <= N <= 255, 1 <= n <= 65535, 0 <= R <= 8, 1 <= gr[r] <= 255 and Q = G + R K >= 1 are the
// caller's to check (pmdi_agreement_create).  trace_row: this add's row of the trace [Q], or null when the trace is full.
hipError_t pmdi_launch_agreement_add(const AgreementArgs &a, double *trace_row, hipStream_t stream)
{
    const long long rows = (long long)a.C * a.K;
    hipLaunchKernelGGL(agreement_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, a.s, rows, a.n, a.np, a.N, a.bytes, a.err);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (a.G > 0 && (e = contingency(a, nullptr, a.N, 0, a.G, stream)) != hipSuccess) return e;
    for (int r = 0; r < a.R; ++r)
        if ((e = contingency(a, a.ref + (size_t)r * a.np, a.gr[r], a.G + r * a.K, a.K, stream)) != hipSuccess) return e;
    long long bi = ((long long)a.C * a.Q + 255) / 256;
    if (bi > (1 << 20)) bi = 1 << 20;                        // (the lanes stride over what is left)
    hipLaunchKernelGGL(agreement_finish_kernel, dim3((unsigned)(bi + (trace_row ? 1 : 0))), dim3(256), 0, stream, a, (unsigned)bi, trace_row);
    return hipGetLastError();
}
