// lane_probe_body.h -- TEST INFRASTRUCTURE ONLY.  One probe body per wave primitive of the lane API of
// particlemdi.jl_amd/csrc/pmdi_sweep2_body.h, written against the PM2_* macros and the pmdi_s2:: names only, so that the same text
// runs on gfx950 (tests/probe/probe.hip: the lane API of the product headers) and on the host (tests/emu/emu_lanes.cpp: the lane API
// of tests/emu/lane_api_emu.h).  Both are held, bit for bit, to the specification of tests/_np_lanes.py.
// Every body is run by one workgroup of 64 lanes, all active, per input vector (PM2_BID() is the vector); every lane writes what it got.
// Include after the lane API.  Nothing under particlemdi.jl_amd/ includes this file.
#pragma once

namespace lane_probe {

typedef unsigned long long u64;

// wave_sum_d, wave_max_d, wave_min_d, prev_lane_d of in[vector][lane]
PM2_DEV void wave_reduce(const double *in, double *sum, double *mx, double *mn, double *prev)
{
    const size_t at = (size_t)PM2_BID() * 64 + (size_t)(PM2_TID() & 63);
    const double v = in[at];
    sum[at] = pmdi_s2::wave_sum_d(v);
    mx[at] = pmdi_s2::wave_max_d(v);
    mn[at] = pmdi_s2::wave_min_d(v);
    prev[at] = pmdi_s2::prev_lane_d(v);
}

// wave_excl_scan_i: the exclusive prefix and the total, as every lane sees them
PM2_DEV void wave_scan(const int *in, int *excl, int *total)
{
    const size_t at = (size_t)PM2_BID() * 64 + (size_t)(PM2_TID() & 63);
    int tot = 0x5A5A5A5A;
    excl[at] = pmdi_s2::wave_excl_scan_i(in[at], tot);
    total[at] = tot;
}

// shfl_d and shfl_i with a source lane per lane: src[vector][lane] in 0..63
PM2_DEV void wave_shfl(const double *vd, const int *vi, const int *src, double *outd, int *outi)
{
    const size_t at = (size_t)PM2_BID() * 64 + (size_t)(PM2_TID() & 63);
    const int s = src[at];
    outd[at] = pmdi_s2::shfl_d(vd[at], s);
    outi[at] = pmdi_s2::shfl_i(vi[at], s);
}

// readlane_i and readlane_u64 with one (wave-uniform) source lane per vector: src[vector]
PM2_DEV void wave_readlane(const int *vi, const u64 *vu, const int *src, int *outi, u64 *outu)
{
    const size_t at = (size_t)PM2_BID() * 64 + (size_t)(PM2_TID() & 63);
    const int s = src[PM2_BID()];
    outi[at] = pmdi_s2::readlane_i(vi[at], s);
    outu[at] = pmdi_s2::readlane_u64(vu[at], s);
}

// popc_below64(bm, p[q]) for nq queries, one per lane
PM2_DEV void popc64(const u64 *bm, const int *p, int nq, int *out)
{
    const int q = PM2_BID() * 64 + (PM2_TID() & 63);
    if (q < nq) out[q] = pmdi_s2::popc_below64(bm, p[q]);
}

// RegArr<int, NN>: every field starts as -1 - i, then set(idx, x) with a run-time index that differs from lane to lane (an index
// outside [0, NN) must change nothing), then every index is read back twice: with a compile-time index into out[vector][lane][i], with a
// run-time one into outrt[vector][lane][i]
template <int NN>
PM2_DEV void regarr(const int *idx, const int *x, int *out, int *outrt)
{
    const size_t at = (size_t)PM2_BID() * 64 + (size_t)(PM2_TID() & 63);
    pmdi_s2::RegArr<int, NN> a;
#pragma unroll
    for (int i = 0; i < NN; ++i) a.set(i, -1 - i);
    a.set(idx[at], x[at]);
#pragma unroll
    for (int i = 0; i < NN; ++i) out[at * NN + i] = a[i];
    const int r0 = idx[at] & (NN - 1);      // a rotation the compiler cannot see through
    for (int i = 0; i < NN; ++i) { const int r = (r0 + i) & (NN - 1); outrt[at * NN + r] = a[r]; }
}

}  // namespace lane_probe
