// pmdi_fixlog.h -- the fixed-point logarithm L of include/pmdi_hip.h on the device, stated once for its three users
// (pmdi_psm_refine_vi.hip, pmdi_partdist.hip, pmdi_partdist_refine.hip).  The 2049 table entries stay in pmdi_vi_log2_table.h;
// every kernel copies them into its own LDS and hands the functions below that copy.
#pragma once
#include <hip/hip_runtime.h>

#define PMDI_FIXLOG_TABLE 2049

// L(x), 1 <= x < 2^62: the exponent, the table entry of the mantissa's first 11 bits and a linear step towards the next entry by
// its following 32 bits.  t1 - t0 < 2^20 and r32 < 2^32: the high word of their 64-bit product is (t1 - t0) r32 >> 32.
__device__ __forceinline__ long long pmdi_fixlog_L(unsigned long long x, const int *T)
{
    const int e = 63 - __clzll((long long)x);
    const unsigned long long f = (x << (62 - e)) - (1ull << 62);
    const unsigned k = (unsigned)(f >> 51);
    const unsigned r32 = (unsigned)((f & ((1ull << 51) - 1ull)) >> 19);
    const int t0 = T[k], t1 = T[k + 1];
    return ((long long)e << 30) + (long long)t0 + (long long)__umulhi((unsigned)(t1 - t0), r32);
}

// s L(s), with 0 L(0) = 0
__device__ __forceinline__ long long pmdi_fixlog_sL(int s, const int *T)
{
    return s > 0 ? (long long)s * pmdi_fixlog_L((unsigned long long)s, T) : 0;
}

// The same L for 1 <= x < 2^32, in 32-bit steps: with m = x << (31 - e) (bit 31 set) the f above is (m - 2^31) << 31, so
// k = f >> 51 = (m - 2^31) >> 20 and r32 = (f & (2^51 - 1)) >> 19 = (m & (2^20 - 1)) << 12.
__device__ __forceinline__ long long pmdi_fixlog_L32(unsigned x, const int *T)
{
    const int e = 31 - __clz((int)x);
    const unsigned m = x << (31 - e);
    const unsigned k = (m & 0x7fffffffu) >> 20;
    const unsigned r32 = (m & 0xfffffu) << 12;
    const int t0 = T[k], t1 = T[k + 1];
    return ((long long)e << 30) + (long long)t0 + (long long)__umulhi((unsigned)(t1 - t0), r32);
}

// v L(v) with 0 L(0) = 0, branch-free: L(1) = 0
__device__ __forceinline__ unsigned long long pmdi_fixlog_vL32(unsigned v, const int *T)
{
    return (unsigned long long)v * (unsigned long long)pmdi_fixlog_L32(v ? v : 1u, T);
}
