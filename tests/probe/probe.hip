// probe.hip -- TEST INFRASTRUCTURE ONLY.  The wave and block primitives of the sweep kernels, one probe kernel each, for gfx950:
//   A  the wave primitives of the lane API (bodies: lane_probe_body.h, shared with the host build of tests/emu/emu_lanes.cpp);
//   B  the block primitives of pmdi_device.h (namespace pmdi_dev: not part of the lane API, so device only);
//   C  the device forms of pmdi_arith.h that the host never runs (uniform01<true>, the device frexp / ldexp / floor of resample_u_at).
// tests/_probe.py compiles this file with the flags of the product library and tests/test_gpu_lanes.py compares what the kernels
// write with the specification of tests/_np_lanes.py.  One workgroup per input vector; every launcher takes device pointers, sizes and
// a stream and returns hipGetLastError().  Not linked into, loaded by or shipped with the product library.
#include <hip/hip_runtime.h>

#include "pmdi_device.h"
#include "pmdi_sweep2_body.h"

#include "lane_probe_body.h"

namespace {

typedef unsigned long long u64;

// ---- A: the wave primitives ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_wave_reduce(const double *in, double *sum, double *mx, double *mn, double *prev)
{
    lane_probe::wave_reduce(in, sum, mx, mn, prev);
}
__global__ void __launch_bounds__(64) k_wave_scan(const int *in, int *excl, int *total) { lane_probe::wave_scan(in, excl, total); }
__global__ void __launch_bounds__(64) k_wave_shfl(const double *vd, const int *vi, const int *src, double *outd, int *outi)
{
    lane_probe::wave_shfl(vd, vi, src, outd, outi);
}
__global__ void __launch_bounds__(64) k_wave_readlane(const int *vi, const u64 *vu, const int *src, int *outi, u64 *outu)
{
    lane_probe::wave_readlane(vi, vu, src, outi, outu);
}
__global__ void __launch_bounds__(64) k_popc64(const u64 *bm, const int *p, int nq, int *out) { lane_probe::popc64(bm, p, nq, out); }
template <int NN>
__global__ void __launch_bounds__(64) k_regarr(const int *idx, const int *x, int *out, int *outrt) { lane_probe::regarr<NN>(idx, x, out, outrt); }

// ---- B: the block primitives of pmdi_device.h ---------------------------------------------------------------------------------------
// two scans in a row on the same scratch (the function's two barriers make that safe), of a[vector][thread] and b[vector][thread]
template <int T>
__global__ void __launch_bounds__(T) k_block_excl_scan(const u64 *a, const u64 *b, u64 *ea, u64 *ta, u64 *eb, u64 *tb)
{
    __shared__ u64 scr[T / 64];
    const size_t at = (size_t)blockIdx.x * T + threadIdx.x;
    u64 tot = 0;
    ea[at] = pmdi_dev::block_excl_scan<T>(a[at], tot, scr);
    ta[at] = tot;
    eb[at] = pmdi_dev::block_excl_scan<T>(b[at], tot, scr);
    tb[at] = tot;
}
// flags[vector][thread]: bit i is flag i
template <int T>
__global__ void __launch_bounds__(T) k_block_flag_scan(const unsigned char *flags, u64 *excl, u64 *total)
{
    __shared__ u64 scr[T / 64];
    const size_t at = (size_t)blockIdx.x * T + threadIdx.x;
    const int f = flags[at];
    u64 tot = 0;
    excl[at] = pmdi_dev::block_flag_scan<T>((f & 1) != 0, (f & 2) != 0, (f & 4) != 0, tot, scr);
    total[at] = tot;
}
// block_max of a, then block_sum2 of (a, b), back to back on the same 48 doubles (the order of PMDI_SWEEP_ESS in pmdi_sweep_body.h)
template <int T>
__global__ void __launch_bounds__(T) k_block_max_sum2(const double *a, const double *b, double *mx, double *sa, double *sb)
{
    __shared__ double scr[48];
    const size_t at = (size_t)blockIdx.x * T + threadIdx.x;
    double x = a[at], y = b[at];
    mx[at] = pmdi_dev::block_max<T>(x, scr);
    pmdi_dev::block_sum2<T>(x, y, scr);
    sa[at] = x;
    sb[at] = y;
}
// mode 0: wave_group, 1: wave_group_lead (lead = the leader's lane), 2: wave_group_capped with `rounds` elections
__global__ void __launch_bounds__(64) k_wave_group(const int *key, const unsigned char *valid, int mode, int rounds, int *lead, int *count)
{
    const size_t at = (size_t)blockIdx.x * 64 + threadIdx.x;
    const int k = key[at];
    const bool v = valid[at] != 0;
    int c = 0x5A5A5A5A, l;
    if (mode == 0) l = pmdi_dev::wave_group(k, v, c) ? 1 : 0;
    else if (mode == 1) l = pmdi_dev::wave_group_lead(k, v, c);
    else l = pmdi_dev::wave_group_capped(k, v, c, rounds) ? 1 : 0;
    lead[at] = l;
    count[at] = c;
}
__global__ void __launch_bounds__(64) k_popc_below(const unsigned *bm, const int *p, int nq, int *out)
{
    const int q = (int)(blockIdx.x * 64 + threadIdx.x);
    if (q < nq) out[q] = pmdi_dev::popc_below(bm, p[q]);
}
// array v of the call: c[off[v] .. off[v + 1]), in place, by thread 0 of workgroup v
__global__ void __launch_bounds__(64) k_jl_cumsum(double *c, const int *off)
{
    if (threadIdx.x == 0) pmdi_dev::jl_cumsum_inplace(c + off[blockIdx.x], off[blockIdx.x + 1] - off[blockIdx.x]);
}

// ---- C: the device forms of pmdi_arith.h --------------------------------------------------------------------------------------------
// tuple t: seed[t], w[t][5] = (iter, pos, k, p, site)
__global__ void __launch_bounds__(256) k_uniform(const u64 *seed, const unsigned *w, int nt, double *mulhi, double *mul64)
{
    const int t = (int)(blockIdx.x * 256 + threadIdx.x);
    if (t >= nt) return;
    const unsigned *c = w + (size_t)t * 5;
    mulhi[t] = pmdi_arith::uniform01<true>(seed[t], c[0], c[1], c[2], c[3], c[4]);
    mul64[t] = pmdi_arith::uniform01<false>(seed[t], c[0], c[1], c[2], c[3], c[4]);
}
// out[i][j] = resample_u_at(u01[i], P, j), j < P
__global__ void __launch_bounds__(256) k_resample_u(const double *u01, int nu, int P, double *out)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)nu * P) return;
    out[t] = pmdi_arith::resample_u_at(u01[t / P], P, (int)(t % P));
}

}  // namespace

#define LP_LAUNCH(kernel_, grid_, block_, ...)                                                                                    \
    do {                                                                                                                          \
        if ((grid_) > 0) hipLaunchKernelGGL(kernel_, dim3((unsigned)(grid_)), dim3((unsigned)(block_)), 0, (hipStream_t)stream, __VA_ARGS__); \
        return hipGetLastError();                                                                                                 \
    } while (0)

extern "C" {

hipError_t lp_wave_reduce(const double *in, double *sum, double *mx, double *mn, double *prev, int nvec, void *stream)
{
    LP_LAUNCH(k_wave_reduce, nvec, 64, in, sum, mx, mn, prev);
}
hipError_t lp_wave_scan(const int *in, int *excl, int *total, int nvec, void *stream) { LP_LAUNCH(k_wave_scan, nvec, 64, in, excl, total); }
hipError_t lp_wave_shfl(const double *vd, const int *vi, const int *src, double *outd, int *outi, int nvec, void *stream)
{
    LP_LAUNCH(k_wave_shfl, nvec, 64, vd, vi, src, outd, outi);
}
hipError_t lp_wave_readlane(const int *vi, const u64 *vu, const int *src, int *outi, u64 *outu, int nvec, void *stream)
{
    LP_LAUNCH(k_wave_readlane, nvec, 64, vi, vu, src, outi, outu);
}
hipError_t lp_popc64(const u64 *bm, const int *p, int *out, int nq, void *stream) { LP_LAUNCH(k_popc64, (nq + 63) / 64, 64, bm, p, nq, out); }
hipError_t lp_regarr(const int *idx, const int *x, int *out, int *outrt, int nvec, int nn, void *stream)
{
    if (nn == 1) LP_LAUNCH(k_regarr<1>, nvec, 64, idx, x, out, outrt);
    if (nn == 2) LP_LAUNCH(k_regarr<2>, nvec, 64, idx, x, out, outrt);
    if (nn == 4) LP_LAUNCH(k_regarr<4>, nvec, 64, idx, x, out, outrt);
    if (nn == 8) LP_LAUNCH(k_regarr<8>, nvec, 64, idx, x, out, outrt);
    return hipErrorInvalidValue;
}

hipError_t lp_block_excl_scan(const u64 *a, const u64 *b, u64 *ea, u64 *ta, u64 *eb, u64 *tb, int nvec, int T, void *stream)
{
    if (T == 256) LP_LAUNCH(k_block_excl_scan<256>, nvec, 256, a, b, ea, ta, eb, tb);
    if (T == 512) LP_LAUNCH(k_block_excl_scan<512>, nvec, 512, a, b, ea, ta, eb, tb);
    if (T == 1024) LP_LAUNCH(k_block_excl_scan<1024>, nvec, 1024, a, b, ea, ta, eb, tb);
    return hipErrorInvalidValue;
}
hipError_t lp_block_flag_scan(const unsigned char *flags, u64 *excl, u64 *total, int nvec, int T, void *stream)
{
    if (T == 256) LP_LAUNCH(k_block_flag_scan<256>, nvec, 256, flags, excl, total);
    if (T == 512) LP_LAUNCH(k_block_flag_scan<512>, nvec, 512, flags, excl, total);
    if (T == 1024) LP_LAUNCH(k_block_flag_scan<1024>, nvec, 1024, flags, excl, total);
    return hipErrorInvalidValue;
}
hipError_t lp_block_max_sum2(const double *a, const double *b, double *mx, double *sa, double *sb, int nvec, int T, void *stream)
{
    if (T == 256) LP_LAUNCH(k_block_max_sum2<256>, nvec, 256, a, b, mx, sa, sb);
    if (T == 512) LP_LAUNCH(k_block_max_sum2<512>, nvec, 512, a, b, mx, sa, sb);
    if (T == 1024) LP_LAUNCH(k_block_max_sum2<1024>, nvec, 1024, a, b, mx, sa, sb);
    return hipErrorInvalidValue;
}
hipError_t lp_wave_group(const int *key, const unsigned char *valid, int *lead, int *count, int nvec, int mode, int rounds, void *stream)
{
    if (mode < 0 || mode > 2) return hipErrorInvalidValue;
    LP_LAUNCH(k_wave_group, nvec, 64, key, valid, mode, rounds, lead, count);
}
hipError_t lp_popc_below(const unsigned *bm, const int *p, int *out, int nq, void *stream)
{
    LP_LAUNCH(k_popc_below, (nq + 63) / 64, 64, bm, p, nq, out);
}
hipError_t lp_jl_cumsum(const int *off, double *c, int narr, void *stream) { LP_LAUNCH(k_jl_cumsum, narr, 64, c, off); }

hipError_t lp_uniform(const u64 *seed, const unsigned *w, double *mulhi, double *mul64, int nt, void *stream)
{
    LP_LAUNCH(k_uniform, (nt + 255) / 256, 256, seed, w, nt, mulhi, mul64);
}
hipError_t lp_resample_u(const double *u01, double *out, int nu, int P, void *stream)
{
    LP_LAUNCH(k_resample_u, ((long long)nu * P + 255) / 256, 256, u01, nu, P, out);
}

}  // extern "C"
