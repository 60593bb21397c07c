// emu_lanes.cpp -- TEST INFRASTRUCTURE ONLY.  The probe bodies of tests/probe/lane_probe_body.h on the lane API of the workgroup
// emulator (lane_api_emu.h), one emulated workgroup of 64 lanes per input vector: the host half of the lane conformance suite
// (tests/_np_lanes.py is the specification, tests/probe/probe.hip the gfx950 half).  The entry points carry the names and the
// argument lists of probe.hip's launchers, on host arrays; the stream is ignored.
#include <cstddef>

#include "lane_api_emu.h"
#include "../../particlemdi.jl_amd/csrc/pmdi_sweep2_body.h"      // popc_below64 and RegArr, on the emulator's lane API

#include "../probe/lane_probe_body.h"

namespace {

typedef unsigned long long u64;

// run `body` (a callable without arguments) on every lane of nblocks workgroups of 64 lanes
template <class F>
void run_blocks(int nblocks, F body)
{
    for (int b = 0; b < nblocks; ++b)
        wavesim::run_block(64, b, 0, [](void *p) { (*(F *)p)(); }, &body, 64 * 1024);
}

}  // namespace

extern "C" {

int lp_wave_reduce(const double *in, double *sum, double *mx, double *mn, double *prev, int nvec, void *)
{
    run_blocks(nvec, [=] { lane_probe::wave_reduce(in, sum, mx, mn, prev); });
    return 0;
}
int lp_wave_scan(const int *in, int *excl, int *total, int nvec, void *)
{
    run_blocks(nvec, [=] { lane_probe::wave_scan(in, excl, total); });
    return 0;
}
int lp_wave_shfl(const double *vd, const int *vi, const int *src, double *outd, int *outi, int nvec, void *)
{
    run_blocks(nvec, [=] { lane_probe::wave_shfl(vd, vi, src, outd, outi); });
    return 0;
}
int lp_wave_readlane(const int *vi, const u64 *vu, const int *src, int *outi, u64 *outu, int nvec, void *)
{
    run_blocks(nvec, [=] { lane_probe::wave_readlane(vi, vu, src, outi, outu); });
    return 0;
}
int lp_popc64(const u64 *bm, const int *p, int *out, int nq, void *)
{
    run_blocks((nq + 63) / 64, [=] { lane_probe::popc64(bm, p, nq, out); });
    return 0;
}
int lp_regarr(const int *idx, const int *x, int *out, int *outrt, int nvec, int nn, void *)
{
    if (nn == 1) run_blocks(nvec, [=] { lane_probe::regarr<1>(idx, x, out, outrt); });
    else if (nn == 2) run_blocks(nvec, [=] { lane_probe::regarr<2>(idx, x, out, outrt); });
    else if (nn == 4) run_blocks(nvec, [=] { lane_probe::regarr<4>(idx, x, out, outrt); });
    else if (nn == 8) run_blocks(nvec, [=] { lane_probe::regarr<8>(idx, x, out, outrt); });
    else return 1;
    return 0;
}

}  // extern "C"
