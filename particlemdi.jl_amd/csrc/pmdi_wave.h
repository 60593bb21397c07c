// pmdi_wave.h -- wave-level primitives on the DPP network of gfx950 (no LDS round trips), device only: the one copy for the general
// kernel (pmdi_device.h) and the settled-chain kernel (the gfx950 lane API of pmdi_sweep2_body.h).  All 64 lanes must be active.
#pragma once

namespace pmdi_wave {

template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xF, 0xF, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double readlane_f64(double v, int l)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
// All-reduce of a double: xor-1 and xor-2 inside quads, half-row and row mirrors give every lane its 16-lane row total; the four row
// totals are read with v_readlane and combined as (r0 op r1) op (r2 op r3).  Every lane returns the same bits.  (max / min: when the
// extremum is a zero and the wave holds zeros of both signs, which of the two comes back is not specified.)
__device__ __forceinline__ double wave_sum_f64(double v)
{
    v += dpp_f64<0xB1>(v);      // quad_perm [1,0,3,2]
    v += dpp_f64<0x4E>(v);      // quad_perm [2,3,0,1]
    v += dpp_f64<0x141>(v);     // row_half_mirror
    v += dpp_f64<0x140>(v);     // row_mirror
    return (readlane_f64(v, 0) + readlane_f64(v, 16)) + (readlane_f64(v, 32) + readlane_f64(v, 48));
}
__device__ __forceinline__ double wave_max_f64(double v)
{
    double t;
    t = dpp_f64<0xB1>(v); v = (t > v) ? t : v;
    t = dpp_f64<0x4E>(v); v = (t > v) ? t : v;
    t = dpp_f64<0x141>(v); v = (t > v) ? t : v;
    t = dpp_f64<0x140>(v); v = (t > v) ? t : v;
    const double r0 = readlane_f64(v, 0), r1 = readlane_f64(v, 16), r2 = readlane_f64(v, 32), r3 = readlane_f64(v, 48);
    const double m01 = (r1 > r0) ? r1 : r0, m23 = (r3 > r2) ? r3 : r2;
    return (m23 > m01) ? m23 : m01;
}
__device__ __forceinline__ double wave_min_f64(double v)
{
    double t;
    t = dpp_f64<0xB1>(v); v = (t < v) ? t : v;
    t = dpp_f64<0x4E>(v); v = (t < v) ? t : v;
    t = dpp_f64<0x141>(v); v = (t < v) ? t : v;
    t = dpp_f64<0x140>(v); v = (t < v) ? t : v;
    const double r0 = readlane_f64(v, 0), r1 = readlane_f64(v, 16), r2 = readlane_f64(v, 32), r3 = readlane_f64(v, 48);
    const double m01 = (r1 < r0) ? r1 : r0, m23 = (r3 < r2) ? r3 : r2;
    return (m23 < m01) ? m23 : m01;
}
// the value of the lane below (lane 0 keeps its own): one DPP shift across the whole wave
__device__ __forceinline__ double prev_lane_f64(double v) { return dpp_f64<0x138>(v); }      // wave_shr:1
// exclusive prefix sum of an int over the wave, and the total (shifts inside the rows of sixteen lanes, then the row totals
// broadcast into the rows above)
__device__ __forceinline__ int wave_excl_scan_i(int v, int &total)
{
    int inc = v;
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x111, 0xF, 0xF, false);      // row_shr:1
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x112, 0xF, 0xF, false);      // row_shr:2
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x114, 0xF, 0xF, false);      // row_shr:4
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x118, 0xF, 0xF, false);      // row_shr:8
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x142, 0xA, 0xF, false);      // row_bcast:15 into rows 1 and 3
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x143, 0xC, 0xF, false);      // row_bcast:31 into rows 2 and 3
    total = __builtin_amdgcn_readlane(inc, 63);
    return inc - v;
}

}  // namespace pmdi_wave
