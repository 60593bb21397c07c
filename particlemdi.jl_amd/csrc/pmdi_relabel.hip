// pmdi_relabel.hip -- the streaming relabelling accumulator (include/pmdi_hip.h, pmdi_relabel_*): every chain starts from a
// random allocation, so label 3 of one chain and label 3 of another are different clusters.  For every retained state of every
// chain this finds the permutation of the N labels that agrees best with a pivot clustering fixed in advance, applies it and
// counts, per dataset and observation, how often each relabelled component was drawn.  An assignment unit is the whole chain
// (shared: one permutation for its K datasets, which keeps every event [c_a = c_b] intact) or one dataset of it.  One add is
// these launches on the accumulator's stream:
//   relabel_rows_kernel     one wavefront per (chain, dataset) row: the int32 labels once, as bytes [np] with MX_PAD for a label
//                           outside 0..N-1 and behind n (the rule of agreement_rows_kernel)
//   relabel_table_kernel    one workgroup per (chain, unit): W[l][g] = #{(k, i) : s[k][i] = l, pivot[k][i] = g}, a product of
//                           one-hot int8 matrices with the observations as the inner dimension (v_mfma_i32_32x32x32_i8); the
//                           four waves share the unit's (dataset, 1 KiB round) items and add their accumulators into one LDS tile
//                           (integer adds: the order does not matter), which goes out to the table in device memory
//   relabel_assign_kernel   one wavefront per (chain, unit): the N x N assignment problem, exactly, by the algorithm of the
//                           header; the cost matrix in LDS up to RL_LDS_N labels, read from the table beyond
//   relabel_count_kernel    one workgroup per (tile of observations, dataset): the tile's counts [label][observation] in LDS,
//                           the chains walked in order, the permutations staged through LDS; every word of alloc has one owner
//   relabel_finish_kernel   one lane per (chain, unit): match_sum, moved; one lane per (chain, dataset, label): w_sum, w_sq
// The tables of a batch of chains are scratch: the first three launches repeat per batch, and nothing depends on its size.
#include <hip/hip_runtime.h>

#include "pmdi_internal.h"
#include "pmdi_onehot.h"            // the fragment types, MX_PAD, mx_wave_sync, mx_wave_sum, mx_onehot, mx_label_row

#pragma clang fp contract(off)      // w_sq is defined with a separate multiply and add (the build passes -ffp-contract=off too)

namespace {

#define RL_CHUNK 1024   // label bytes of one side a wave stages per round: 16 per lane
#define RL_PERMS 32     // chains whose permutations the count kernel stages per round
#define RL_LDS_N 192    // the largest N whose cost matrix the assignment stages in LDS: 144 KiB of the CU's 160

__global__ void __launch_bounds__(256) relabel_rows_kernel(const int *__restrict__ s, long long n_rows, long long n, int np, int N,
                                                           unsigned char *__restrict__ out, int *__restrict__ err)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row = (long long)blockIdx.x * 4 + wave;
    if (row >= n_rows) return;                               // (the same in every lane of a wave; no barrier below)
    const bool bad = mx_label_row(s + row * n, n, np, N, (unsigned *)(out + row * np), lane);
    if (lane == 0 && bad) *err = 1;
}

// tables[chain][u][l][g], chain = blockIdx.x of the batch whose label bytes start at `bytes`, u = blockIdx.y of U = gridDim.y
// units: the datasets k0 = u Ku .. k0 + Ku - 1 (shared: Ku = K, U = 1; else Ku = 1, U = K).  The fragments are those of
// agreement_contingency_kernel: lane (r = lane & 31, h = lane >> 5) holds [s_i == label r] for the 16 observations of half h
// as the A fragment and [pivot_i == label r] as the B fragment.  NT = 32-label tiles per side of one pass (1: N <= 32, else 2);
// the passes run over the pairs of label blocks.  Entry e of a lane's accumulator is row (e & 3) + 8 (e >> 2) + 4 h, column r
// of the 32 x 32 tile.  An observation with MX_PAD on either side (no label, or not part of the matching) is in no cell.
template <int NT>
__global__ void __launch_bounds__(256) relabel_table_kernel(const unsigned char *__restrict__ bytes, const unsigned char *__restrict__ pivot,
                                                            int K, int Ku, int np, int N, int *__restrict__ tables)
{
    __shared__ __attribute__((aligned(16))) mx_v4u stage[4][2][RL_CHUNK / 16];
    __shared__ int tile[32 * NT][32 * NT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const long long chain = blockIdx.x;
    const int u = blockIdx.y, U = gridDim.y, k0 = u * Ku;
    const int chunks = (np + RL_CHUNK - 1) / RL_CHUNK, items = Ku * chunks;
    int *out = tables + (chain * U + u) * N * N;
    mx_v4u *sx = stage[wave][0], *sy = stage[wave][1];
    const int nb = (N + 32 * NT - 1) / (32 * NT);
    for (int bx = 0; bx < nb; ++bx)
        for (int by = 0; by < nb; ++by) {
            for (int i = tid; i < 32 * NT * 32 * NT; i += 256) (&tile[0][0])[i] = 0;
            __syncthreads();
            unsigned rep_x[NT], one_x[NT], rep_y[NT], one_y[NT];
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const unsigned lx = (unsigned)(32 * NT * bx + 32 * i + r), ly = (unsigned)(32 * NT * by + 32 * i + r);
                rep_x[i] = lx * 0x01010101u; one_x[i] = lx < (unsigned)N ? 0x01010101u : 0u;
                rep_y[i] = ly * 0x01010101u; one_y[i] = ly < (unsigned)N ? 0x01010101u : 0u;
            }
            mx_v16i acc[NT][NT];
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[i][j][e] = 0;
            for (int item = wave; item < items; item += 4) {
                const int k = k0 + item / chunks, c0 = (item % chunks) * RL_CHUNK;
                const mx_v4u *xp = (const mx_v4u *)(bytes + (chain * K + k) * np);
                const mx_v4u *yp = (const mx_v4u *)(pivot + (long long)k * np);
                const int left = np - c0;                    // a multiple of 32
                mx_v4u vx = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, vy = vx;
                if (16 * lane < left) { vx = xp[(c0 >> 4) + lane]; vy = yp[(c0 >> 4) + lane]; }
                mx_wave_sync();                              // the steps of the last round have read the buffers
                sx[lane] = vx;
                sy[lane] = vy;
                mx_wave_sync();
                const int steps = left < RL_CHUNK ? left >> 5 : RL_CHUNK / 32;
                for (int st = 0; st < steps; ++st) {
                    const mx_v4u x16 = sx[2 * st + h], y16 = sy[2 * st + h];
                    mx_v4i fx[NT], fy[NT];
#pragma unroll
                    for (int i = 0; i < NT; ++i) { fx[i] = mx_onehot(x16, rep_x[i], one_x[i]); fy[i] = mx_onehot(y16, rep_y[i], one_y[i]); }
#pragma unroll
                    for (int i = 0; i < NT; ++i)
#pragma unroll
                        for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fx[i], fy[j], acc[i][j], 0, 0, 0);
                }
            }
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) atomicAdd(&tile[32 * i + (e & 3) + 8 * (e >> 2) + 4 * h][32 * j + r], acc[i][j][e]);
            __syncthreads();
            for (int i = tid; i < 32 * NT * 32 * NT; i += 256) {
                const int l = 32 * NT * bx + i / (32 * NT), g = 32 * NT * by + i % (32 * NT);
                if (l < N && g < N) out[l * N + g] = tile[i / (32 * NT)][i % (32 * NT)];
            }
            __syncthreads();                                 // (the tile is zeroed again for the next pair of blocks)
        }
}

// Problem b = blockIdx.x: W = tables[b] [N][N]; perm[b][l] = sigma(l) maximises sum_l W[l][sigma(l)], value[b] is that sum, and
// moved[b] (where asked for) is 1 iff sigma(l) != l for a label l whose row of W is not all zero.  The algorithm is the one
// pinned in include/pmdi_hip.h, in Int64: rows are inserted in order; a row's insertion grows an alternating tree from the
// dummy column N by shortest reduced cost.  Lane `lane` owns the columns j = lane + 64 t, t < CPL (1, 2 or 4 columns per
// lane): their v, minv and `used` live in its registers; u (by row), p (row matched to a column, p[N] the row being inserted)
// and way (by column) live in LDS, every word written by the column's or the row's one owner.  The column choice is a
// reduction over the wave on the pair (minv, j), compared lexicographically: the smallest j among the smallest minv.
// STAGED: the matrix is copied to LDS first; else every row is read from the table (the values are the same).
template <int CPL, bool STAGED>
__global__ void __launch_bounds__(64) relabel_assign_kernel(const int *__restrict__ tables, int N, unsigned char *__restrict__ perm,
                                                            long long *__restrict__ value, int *__restrict__ moved)
{
    extern __shared__ int rl_dyn[];                          // STAGED: W [N][N]
    __shared__ long long u[256];
    __shared__ int p[257], way[256];
    __shared__ int occupied[256];
    const int lane = threadIdx.x;
    const long long b = blockIdx.x;
    const int *W = tables + b * N * N;
    if (STAGED)
        for (int i = lane; i < N * N; i += 64) rl_dyn[i] = W[i];
    auto w_at = [&](int i) -> long long { return (long long)(STAGED ? rl_dyn[i] : W[i]); };
    for (int j = lane; j <= N; j += 64) p[j] = -1;
    for (int j = lane; j < N; j += 64) { u[j] = 0; occupied[j] = 0; }
    long long v[CPL];
#pragma unroll
    for (int t = 0; t < CPL; ++t) v[t] = 0;
    mx_wave_sync();
    for (int i = 0; i < N; ++i) {
        long long minv[CPL];
        bool used[CPL];
#pragma unroll
        for (int t = 0; t < CPL; ++t) { minv[t] = 0x7fffffffffffffffLL; used[t] = false; }
        int j0 = N, i0 = i;                                  // (p[N] = i: kept in i0, the dummy column is never read back)
        for (;;) {                                           // j0, i0 and the exit are the same in every lane
#pragma unroll
            for (int t = 0; t < CPL; ++t) used[t] = used[t] || j0 == lane + 64 * t;
            const long long ui0 = u[i0];
            long long best = 0x7fffffffffffffffLL;
            int best_j = 0x7fffffff;
#pragma unroll
            for (int t = 0; t < CPL; ++t) {                  // ascending j within the lane: a tie keeps the smaller one
                const int j = lane + 64 * t;
                if (j < N && !used[t]) {
                    const long long cur = -w_at(i0 * N + j) - ui0 - v[t];
                    if (cur < minv[t]) { minv[t] = cur; way[j] = j0; }
                    if (minv[t] < best) { best = minv[t]; best_j = j; }
                }
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)(unsigned long long)best, off);
                const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)((unsigned long long)best >> 32), off);
                const long long ob = (long long)(((unsigned long long)hi << 32) | lo);
                const int oj = __shfl_xor(best_j, off);
                if (ob < best || (ob == best && oj < best_j)) { best = ob; best_j = oj; }
            }
            const long long delta = best;                    // (a column is always left: at most i of the N are matched)
#pragma unroll
            for (int t = 0; t < CPL; ++t) {
                const int j = lane + 64 * t;
                if (j < N) {
                    if (used[t]) { u[p[j]] += delta; v[t] -= delta; }      // (the rows of the used columns differ, and from i)
                    else minv[t] -= delta;
                }
            }
            if (lane == 0) u[i] += delta;                    // the dummy column is used from the start, and holds row i
            mx_wave_sync();
            j0 = best_j;
            i0 = p[j0];
            if (i0 < 0) break;
        }
        if (lane == 0) {                                     // augment along way[] back to the dummy column
            int j = j0;
            do {
                const int j1 = way[j];
                p[j] = j1 == N ? i : p[j1];
                j = j1;
            } while (j != N);
        }
        mx_wave_sync();
    }
    long long val = 0;
#pragma unroll
    for (int t = 0; t < CPL; ++t) {
        const int j = lane + 64 * t;
        if (j < N) {
            const int l = p[j];
            perm[b * N + l] = (unsigned char)j;
            way[l] = j;                                      // sigma, for the lanes that own other rows
            val += w_at(l * N + j);
        }
    }
    val = (long long)mx_wave_sum((unsigned long long)val);
    if (lane == 0) value[b] = val;
    if (moved) {
        for (int i = lane; i < N * N; i += 64)
            if (w_at(i) != 0) occupied[i / N] = 1;           // (every writer writes the same 1)
        mx_wave_sync();
        int mv = 0;
        for (int l = lane; l < N; l += 64) mv |= (occupied[l] && way[l] != l) ? 1 : 0;
        mv = __any(mv);
        if (lane == 0) moved[b] = mv ? 1 : 0;
    }
}

// alloc[k][i][sigma_c(s[c][k][i])] += 1 over the C chains, k = blockIdx.y, for the tile of TW = blockDim.x observations from
// i0 = blockIdx.x TW on: thread t owns observation i0 + t and its column of the counts cnt[label][t] in LDS (the lanes of a
// wave fall on consecutive banks), so nothing is atomic.  The chains are walked in rounds of RL_PERMS: their permutations are
// staged in LDS, then eight label bytes are in flight per thread.  MX_PAD counts nowhere.  At the end the tile is added to
// alloc, the words of [i][g] in order: this workgroup is the only one that touches them.
__global__ void __launch_bounds__(256) relabel_count_kernel(const unsigned char *__restrict__ bytes, const unsigned char *__restrict__ perm,
                                                            int C, int K, int U, int N, int np, long long n, int *__restrict__ alloc)
{
    extern __shared__ int rl_dyn[];                          // cnt [N][TW], then the permutations of a round [RL_PERMS][N] bytes
    const int TW = blockDim.x, t = threadIdx.x, k = blockIdx.y, u = U == 1 ? 0 : k;
    const long long i0 = (long long)blockIdx.x * TW, i = i0 + t;
    int *cnt = rl_dyn;
    unsigned char *sp = (unsigned char *)(rl_dyn + N * TW);
    for (int j = t; j < N * TW; j += TW) cnt[j] = 0;
    const bool mine = i < n;
    const unsigned char *col = bytes + (long long)k * np + (mine ? i : n - 1);       // (clamped: no load sits under a branch)
    for (int c0 = 0; c0 < C; c0 += RL_PERMS) {
        const int nc = C - c0 < RL_PERMS ? C - c0 : RL_PERMS;
        __syncthreads();                                     // the last round has read sp (and the counts are zero)
        for (int j = t; j < nc * N; j += TW) sp[j] = perm[((long long)(c0 + j / N) * U + u) * N + j % N];
        __syncthreads();
        for (int cc = 0; cc < nc; cc += 8) {
            unsigned l[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int c = cc + q < nc ? cc + q : nc - 1;
                l[q] = col[(long long)(c0 + c) * K * np];
            }
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (mine && cc + q < nc && l[q] != MX_PAD) cnt[(int)sp[(cc + q) * N + l[q]] * TW + t] += 1;
        }
    }
    __syncthreads();
    const int w = n - i0 < TW ? (int)(n - i0) : TW;
    int *dst = alloc + ((long long)k * n + i0) * N;
    for (int j = t; j < w * N; j += TW) dst[j] += cnt[(j % N) * TW + j / N];
}

// lanes 0 .. C U - 1: match_sum += value, moved += flag; lanes 0 .. C K N - 1 of an add with Pi: the weight of label l of
// (chain, dataset) goes to component sigma(l), which no other lane of that (chain, dataset) writes
__global__ void __launch_bounds__(256) relabel_finish_kernel(RelabelArgs a)
{
    const long long units = (long long)a.C * a.U, words = a.Pi ? (long long)a.C * a.K * a.N : 0;
    const long long stride = (long long)gridDim.x * 256;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < units || idx < words; idx += stride) {
        if (idx < units) { a.match_sum[idx] += a.value[idx]; a.moved[idx] += a.flag[idx]; }
        if (idx < words) {
            const int l = (int)(idx % a.N);
            const long long ck = idx / a.N;
            const int k = (int)(ck % a.K);
            const long long c = ck / a.K;
            const long long o = ck * a.N + a.perm[(c * a.U + (a.U == 1 ? 0 : k)) * a.N + l];
            const double x = a.Pi[idx];
            a.w_sum[o] = a.w_sum[o] + x;
            a.w_sq[o] = a.w_sq[o] + x * x;
        }
    }
}

template <int CPL, bool STAGED>
hipError_t launch_assign(const int *tables, long long B, int N, unsigned char *perm, long long *value, int *moved, hipStream_t stream)
{
    const size_t lds = STAGED ? (size_t)N * N * 4 : 0;
    auto fn = relabel_assign_kernel<CPL, STAGED>;
    if (lds > 65536 - 8192) {                                // (beyond the default limit of LDS, with the kernel's own 5 KiB of arrays)
        hipError_t e = hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(fn, dim3((unsigned)B), dim3(64), lds, stream, tables, N, perm, value, moved);
    return hipGetLastError();
}

}  // namespace

// observations per workgroup of relabel_count_kernel: N x tile counts fit the LDS beside the staged permutations
int pmdi_relabel_tile(int N) { return N <= 128 ? 256 : 128; }

// tables [B][N][N] int32, perm [B][N], value [B], moved [B] or null: device arrays.  1 <= B <= INT32_MAX and 2 <= N <= 255 are
// the caller's to check.
hipError_t pmdi_launch_relabel_assign(const int *tables, long long B, int N, unsigned char *perm, long long *value, int *moved,
                                      hipStream_t stream)
{
    if (N <= 64) return launch_assign<1, true>(tables, B, N, perm, value, moved, stream);
    if (N <= 128) return launch_assign<2, true>(tables, B, N, perm, value, moved, stream);
    if (N <= RL_LDS_N) return launch_assign<4, true>(tables, B, N, perm, value, moved, stream);
    return launch_assign<4, false>(tables, B, N, perm, value, moved, stream);
}

// 1 <= C, 1 <= K <= PMDI_KMAX_I, 2 <= N <= 255, 1 <= n <= 65535, 1 <= Cb <= C are the caller's to check (pmdi_relabel_create).
hipError_t pmdi_launch_relabel_add(const RelabelArgs &a, hipStream_t stream)
{
    const long long rows = (long long)a.C * a.K;
    hipLaunchKernelGGL(relabel_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, a.s, rows, a.n, a.np, a.N, a.bytes, a.err);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int Ku = a.U == 1 ? a.K : 1;
    for (int c0 = 0; c0 < a.C; c0 += a.Cb) {
        const int nb = a.C - c0 < a.Cb ? a.C - c0 : a.Cb;
        const unsigned char *bytes = a.bytes + (size_t)c0 * a.K * a.np;
        if (a.N <= 32)
            hipLaunchKernelGGL(relabel_table_kernel<1>, dim3((unsigned)nb, (unsigned)a.U), dim3(256), 0, stream, bytes, a.pivot, a.K, Ku, a.np, a.N, a.tables);
        else
            hipLaunchKernelGGL(relabel_table_kernel<2>, dim3((unsigned)nb, (unsigned)a.U), dim3(256), 0, stream, bytes, a.pivot, a.K, Ku, a.np, a.N, a.tables);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        const size_t at = (size_t)c0 * a.U;
        if ((e = pmdi_launch_relabel_assign(a.tables, (long long)nb * a.U, a.N, a.perm + at * a.N, a.value + at, a.flag + at, stream)) != hipSuccess) return e;
    }
    const int TW = pmdi_relabel_tile(a.N);
    const size_t lds = (size_t)a.N * TW * 4 + (size_t)RL_PERMS * a.N;
    if (lds > 65536) {
        e = hipFuncSetAttribute((const void *)relabel_count_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(relabel_count_kernel, dim3((unsigned)((a.n + TW - 1) / TW), (unsigned)a.K), dim3(TW), lds, stream,
                       (const unsigned char *)a.bytes, (const unsigned char *)a.perm, a.C, a.K, a.U, a.N, a.np, a.n, a.alloc);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    long long most = (long long)a.C * a.U;
    if (a.Pi && (long long)a.C * a.K * a.N > most) most = (long long)a.C * a.K * a.N;
    long long blocks = (most + 255) / 256;
    if (blocks > (1 << 20)) blocks = 1 << 20;                // (the lanes stride over what is left)
    hipLaunchKernelGGL(relabel_finish_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
    return hipGetLastError();
}
