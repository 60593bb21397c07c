// pmdi_hclust.hip -- get_consensus_allocations (src/output_analysis/consensus_map.jl:92-105) on the MI355X:
// distance matrix from the co-clustering counts, agglomerative clustering by the nearest-neighbour chain with
// Lance-Williams updates (one persistent workgroup per matrix), and the host-side sort / renumbering / cutree.
// The interface, the tie rule and the numbering are specified in include/pmdi_hip.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <new>
#include <numeric>
#include <vector>

#include "../../include/pmdi_hip.h"
#include "pmdi_psm_device.h"

int pmdi_set_error(int code, const char *fmt, ...);   // pmdi_api.cpp
int pmdi_psm_shared_args(const char *who, int64_t S, int32_t K, int64_t n, int32_t which, bool cand, int64_t B, int64_t ld);   // pmdi_api.cpp

namespace {

constexpr int HC_THREADS = 1024;                 // one workgroup = 16 waves
constexpr int HC_WAVES = HC_THREADS / 64;

// ---- (a) distances from counts --------------------------------------------------------------------------
// One thread per element.  The counts are symmetric integers, so element (r, c) reads counts[k][r][c] itself; the
// arithmetic is that of psm.psm_rows (consensus_map.jl:53, :59): p_k = count / S, Overall o = 0.0 + p_0 / K + ...
__global__ void pmdi_psm_distance_kernel(const int *__restrict__ counts, double S, int K, long long n, int which,
                                         double *__restrict__ out)
{
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long r = blockIdx.y;
    if (c >= n) return;
    double d = 0.0;
    if (r != c) {
        if (which < K) {
            d = 1.0 - (double)psm_count(counts, which, n, r, c) / S;
        } else {
            double o = 0.0;
            for (int k = 0; k < K; ++k) o += ((double)psm_count(counts, k, n, r, c) / S) / (double)K;
            d = 1.0 - o;
        }
    }
    out[r * n + c] = d;
}

// ---- check + Symmetric(., :L) ---------------------------------------------------------------------------
// Column-major: element (i, j) lives at i + n * j.  The lower triangle (i > j) is read and checked, the upper
// triangle is overwritten with its mirror image, the diagonal with 0.  Nobody reads what somebody else writes.
__global__ void pmdi_hclust_prepare_kernel(double *dist, long long n, int *bad)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;     // fast index
    const long long j = blockIdx.y;
    double *D = dist + (long long)blockIdx.z * n * n;
    if (i >= n) return;
    if (i > j) {
        const double v = D[i + n * j];
        if (!(v >= 0.0) || v > 1.79769313486231570e308) bad[blockIdx.z] = 1;          // NaN, negative, +inf
    } else if (i < j) {
        D[i + n * j] = D[j + n * i];
    } else {
        D[i + n * j] = 0.0;
    }
}

// ---- (b) nearest-neighbour chain ------------------------------------------------------------------------
// i is the lower slot of the merged pair, j the higher; k any other live cluster
__device__ __forceinline__ double lance_williams(int linkage, double dik, double djk, double dij, int ni, int nj, int nk)
{
    switch (linkage) {
    case PMDI_LINK_SINGLE: return dik < djk ? dik : djk;
    case PMDI_LINK_COMPLETE: return dik > djk ? dik : djk;
    case PMDI_LINK_AVERAGE: return ((double)ni * dik + (double)nj * djk) / (double)(ni + nj);
    default: {      // PMDI_LINK_WARD on distances (not squared), as the reference passes them
        const double t = (double)(ni + nk) * (dik * dik) + (double)(nj + nk) * (djk * djk) - (double)nk * (dij * dij);
        return sqrt(t / (double)(ni + nj + nk));
    }
    }
}

// (value, key) lexicographic minimum; key = -1 for the chain's predecessor (it wins ties), the slot index otherwise
__device__ __forceinline__ void take_min(double &v, int &k, double v2, int k2)
{
    if (v2 < v || (v2 == v && k2 < k)) { v = v2; k = k2; }
}

// One workgroup per matrix.  The matrix is full and symmetric in global memory; a merge rewrites row AND column of
// the surviving slot, so every nearest-neighbour search is one coalesced row read.  size[k] == 0 marks a slot whose
// cluster was merged away; its row and column are never read again.  All control flow is uniform over the workgroup.
__global__ void __launch_bounds__(HC_THREADS)
pmdi_hclust_kernel(double *dist, int n, int linkage, int *iscratch, double *heights)
{
    const long long nn = n;
    double *D = dist + (long long)blockIdx.x * nn * nn;
    int *size = iscratch + (long long)blockIdx.x * 4 * nn;
    int *chain = size + nn, *mlo = chain + nn, *mhi = mlo + nn;
    double *mh = heights + (long long)blockIdx.x * nn;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    __shared__ double s_v[HC_WAVES];
    __shared__ int s_k[HC_WAVES];
    __shared__ int s_tip, s_prev;

    for (int k = tid; k < n; k += HC_THREADS) size[k] = 1;
    int len = 0, first = 0;
    __syncthreads();

    for (int nm = 0; nm < n - 1;) {
        if (tid == 0) {
            if (len == 0) {                                  // a new chain starts at the lowest live slot
                while (size[first] == 0) ++first;
                chain[0] = first;
            }
            const int l = len == 0 ? 1 : len;
            s_tip = chain[l - 1];
            s_prev = l >= 2 ? chain[l - 2] : -1;
        }
        if (len == 0) len = 1;
        __syncthreads();
        const int tip = s_tip, prev = s_prev;
        const double *row = D + (long long)tip * nn;

        double bv = std::numeric_limits<double>::infinity();
        int bk = 0x7fffffff;
        for (int j = tid; j < n; j += HC_THREADS)
            if (j != tip && size[j] > 0) take_min(bv, bk, row[j], j == prev ? -1 : j);
        for (int off = 32; off > 0; off >>= 1) {
            const double v2 = __shfl_xor(bv, off);
            const int k2 = __shfl_xor(bk, off);
            take_min(bv, bk, v2, k2);
        }
        if (lane == 0) { s_v[wave] = bv; s_k[wave] = bk; }
        __syncthreads();
        bv = s_v[0]; bk = s_k[0];
        for (int w = 1; w < HC_WAVES; ++w) take_min(bv, bk, s_v[w], s_k[w]);

        if (bk != -1) {                                      // not reciprocal: the chain grows
            if (tid == 0) chain[len] = bk;
            ++len;
            __syncthreads();                                 // s_v / s_k / s_tip are rewritten in the next round
            continue;
        }
        // tip and prev are reciprocal nearest neighbours: merge them into the higher slot
        const int lo = tip < prev ? tip : prev, hi = tip < prev ? prev : tip;
        const int ni = size[lo], nj = size[hi];
        const double dij = bv;
        const double *rlo = D + (long long)lo * nn;
        double *rhi = D + (long long)hi * nn;
        for (int k = tid; k < n; k += HC_THREADS) {
            const int nk = size[k];
            if (k == lo || k == hi || nk == 0) continue;
            const double v = lance_williams(linkage, rlo[k], rhi[k], dij, ni, nj, nk);
            rhi[k] = v;
            D[(long long)k * nn + hi] = v;
        }
        __syncthreads();                                     // every size[] read above precedes the update below
        if (tid == 0) {
            size[hi] = ni + nj;
            size[lo] = 0;
            mlo[nm] = lo; mhi[nm] = hi; mh[nm] = dij;
        }
        ++nm;
        len -= 2;
        __syncthreads();
    }
}

int hip_fail(hipError_t e, const char *what)
{
    return pmdi_set_error(e == hipErrorOutOfMemory ? PMDI_E_MEMORY : PMDI_E_DEVICE, "%s: %s", what, hipGetErrorString(e));
}

struct DevMem {
    void *p = nullptr;
    ~DevMem() { if (p) (void)hipFree(p); }
};

// chain-order merges (slot pairs) -> stable sort by height, hclust numbering, leaf order
void finish_dendrogram(long long n, const int *lo, const int *hi, const double *h, int64_t *merges, double *heights, int64_t *order)
{
    const long long m = n - 1;
    std::vector<long long> idx(m), parent(n), cid(n);
    std::iota(idx.begin(), idx.end(), 0LL);
    std::stable_sort(idx.begin(), idx.end(), [&](long long a, long long b) { return h[a] < h[b]; });
    for (long long i = 0; i < n; ++i) { parent[i] = i; cid[i] = -(i + 1); }
    auto find = [&](long long x) {
        while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
        return x;
    };
    for (long long r = 0; r < m; ++r) {
        const long long a = find(lo[idx[r]]), b = find(hi[idx[r]]);
        merges[r] = cid[a];                  // column-major (n-1) x 2
        merges[r + m] = cid[b];
        heights[r] = h[idx[r]];
        parent[a] = b;
        cid[b] = r + 1;
    }
    // leaves in depth-first order from the last row, first column before second
    std::vector<long long> stack;
    long long at = 0;
    stack.push_back(m);
    while (!stack.empty()) {
        const long long v = stack.back();
        stack.pop_back();
        if (v < 0) { order[at++] = -v; continue; }
        stack.push_back(merges[v - 1 + m]);
        stack.push_back(merges[v - 1]);
    }
}

}  // namespace

extern "C" {

int pmdi_psm_distance_device(int32_t device, const int32_t *counts, int64_t S, int32_t K, int64_t n, int32_t which,
                             double *dist_out, void *stream)
{
    if (!counts || !dist_out) return pmdi_set_error(PMDI_E_ARG, "pmdi_psm_distance_device: null argument");
    const int rc = pmdi_psm_shared_args("pmdi_psm_distance_device", S, K, n, which, false, 0, 0);
    if (rc) return rc;
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    hipLaunchKernelGGL(pmdi_psm_distance_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)n), dim3(256), 0, (hipStream_t)stream,
                       counts, (double)S, K, (long long)n, which, dist_out);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "psm-distance launch");
    return PMDI_OK;
}

int pmdi_hclust_device(int32_t device, double *dist, int32_t B, int64_t n, int32_t linkage, int64_t *merges_out,
                       double *heights_out, int64_t *order_out, void *stream)
{
    if (!dist || !order_out || (n > 1 && (!merges_out || !heights_out)))
        return pmdi_set_error(PMDI_E_ARG, "pmdi_hclust_device: null argument");
    if (B < 1 || B > 65535 || n < 1 || n > 65535)
        return pmdi_set_error(PMDI_E_ARG, "pmdi_hclust_device: B=%d n=%lld outside 1..65535", B, (long long)n);
    if (linkage < PMDI_LINK_SINGLE || linkage > PMDI_LINK_WARD)
        return pmdi_set_error(PMDI_E_ARG, "pmdi_hclust_device: linkage=%d is not one of PMDI_LINK_*", linkage);
    if (n == 1) {
        for (int b = 0; b < B; ++b) order_out[b] = 1;
        return PMDI_OK;
    }
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    hipStream_t st = (hipStream_t)stream;
    const long long m = n - 1;
    DevMem isc, hsc, bad;
    if ((e = hipMalloc(&isc.p, (size_t)B * 4 * n * sizeof(int))) != hipSuccess) return hip_fail(e, "hipMalloc(scratch)");
    if ((e = hipMalloc(&hsc.p, (size_t)B * n * sizeof(double))) != hipSuccess) return hip_fail(e, "hipMalloc(scratch)");
    if ((e = hipMalloc(&bad.p, (size_t)B * sizeof(int))) != hipSuccess) return hip_fail(e, "hipMalloc(scratch)");
    if ((e = hipMemsetAsync(bad.p, 0, (size_t)B * sizeof(int), st)) != hipSuccess) return hip_fail(e, "hipMemsetAsync");

    hipLaunchKernelGGL(pmdi_hclust_prepare_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)n, (unsigned)B), dim3(256), 0, st,
                       dist, (long long)n, (int *)bad.p);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "hclust check launch");
    std::vector<int> hbad(B);
    if ((e = hipMemcpyAsync(hbad.data(), bad.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st)) != hipSuccess) return hip_fail(e, "hipMemcpyAsync");
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
    for (int b = 0; b < B; ++b)
        if (hbad[b])
            return pmdi_set_error(PMDI_E_DATA, "pmdi_hclust_device: matrix %d holds a distance that is NaN, infinite or negative", b);

    hipLaunchKernelGGL(pmdi_hclust_kernel, dim3((unsigned)B), dim3(HC_THREADS), 0, st, dist, (int)n, (int)linkage, (int *)isc.p, (double *)hsc.p);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "hclust launch");
    std::vector<int> hi_all;
    std::vector<double> hh;
    try {
        hi_all.resize((size_t)B * 4 * n);
        hh.resize((size_t)B * n);
    } catch (const std::bad_alloc &) {
        (void)hipStreamSynchronize(st);
        return pmdi_set_error(PMDI_E_MEMORY, "out of host memory");
    }
    if ((e = hipMemcpyAsync(hi_all.data(), isc.p, hi_all.size() * sizeof(int), hipMemcpyDeviceToHost, st)) != hipSuccess) return hip_fail(e, "hipMemcpyAsync");
    if ((e = hipMemcpyAsync(hh.data(), hsc.p, hh.size() * sizeof(double), hipMemcpyDeviceToHost, st)) != hipSuccess) return hip_fail(e, "hipMemcpyAsync");
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(e, "hclust kernel");
    try {
        for (int b = 0; b < B; ++b) {
            const int *base = hi_all.data() + (size_t)b * 4 * n;
            finish_dendrogram(n, base + 2 * n, base + 3 * n, hh.data() + (size_t)b * n, merges_out + (size_t)b * 2 * m,
                              heights_out + (size_t)b * m, order_out + (size_t)b * n);
        }
    } catch (const std::bad_alloc &) {
        return pmdi_set_error(PMDI_E_MEMORY, "out of host memory");
    }
    return PMDI_OK;
}

int pmdi_cutree(int64_t n, const int64_t *merges, const double *heights, int64_t k, double h, int64_t *labels_out)
{
    if (n < 1 || !labels_out || (n > 1 && (!merges || !heights))) return pmdi_set_error(PMDI_E_ARG, "pmdi_cutree: bad argument");
    const bool by_k = k != -1, by_h = !std::isnan(h);
    if (!by_k && !by_h)
        return pmdi_set_error(PMDI_E_ARG, "You must specify either k (number of clusters) or h (height to cut dendrogram)");
    if (by_k && (k < 1 || k > n)) return pmdi_set_error(PMDI_E_ARG, "pmdi_cutree: k=%lld outside 1..n=%lld", (long long)k, (long long)n);
    const int64_t m = n - 1;
    int64_t apply = 0;
    if (by_k) apply = n - k;                                 // k wins when both are given (consensus_map.jl:99-103)
    else while (apply < m && heights[apply] <= h) ++apply;
    try {
        std::vector<int64_t> parent(n), rep(m > 0 ? m : 1), lab(n, 0);
        for (int64_t i = 0; i < n; ++i) parent[i] = i;
        auto find = [&](int64_t x) {
            while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
            return x;
        };
        for (int64_t r = 0; r < apply; ++r) {
            int64_t root[2];
            for (int c = 0; c < 2; ++c) {
                const int64_t v = merges[r + c * m];
                if (v < 0 && v >= -n) root[c] = find(-v - 1);
                else if (v >= 1 && v <= r) root[c] = find(rep[v - 1]);
                else return pmdi_set_error(PMDI_E_ARG, "pmdi_cutree: merges[%lld, %d] = %lld is not -n..-1 or an earlier row", (long long)r + 1, c + 1, (long long)v);
            }
            parent[root[0]] = root[1];
            rep[r] = root[1];
        }
        int64_t next = 0;
        for (int64_t i = 0; i < n; ++i) {                    // numbered 1.. in order of first appearance
            const int64_t r = find(i);
            if (lab[r] == 0) lab[r] = ++next;
            labels_out[i] = lab[r];
        }
    } catch (const std::bad_alloc &) {
        return pmdi_set_error(PMDI_E_MEMORY, "out of host memory");
    }
    return PMDI_OK;
}

}  // extern "C"
