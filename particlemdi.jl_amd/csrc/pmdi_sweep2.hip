// pmdi_sweep2.hip -- the conditional-SMC sweep for settled chains as a gfx950 kernel: the device code is pmdi_sweep2_body.h (design
// notes there and in DESIGN.md); this file instantiates it per (datasets, particles per lane) and launches it.
// Compile with -ffp-contract=off.
// The general sweep kernel's device code: a chain this kernel's tables no longer hold is carried on by it IN PLACE -- same workgroup,
// same dynamic LDS (the launch asks for the larger of the two layouts), from the observation of the hand-over -- instead of
// waiting for another launch behind this one.
// (-DPM2_NO_RESUME_GENERAL: tests/test_build_budget.py measures this kernel's own spills -- the compiler's figure folds callees in)
#ifndef PM2_NO_RESUME_GENERAL
#define PMDI_BSLOT_FROM_TICKET 1
#include "pmdi_sweep_body.h"
template <int K, int NW>
__device__ __noinline__ void pmdi_resume_general(const SweepArgs *ap)
{
    pmdi_sweep_body<64 * NW, 2, K == 1, false, true>(ap);
}
#define PM2_RESUME_GENERAL(K_, NW_, ap_) pmdi_resume_general<K_, NW_>(ap_)
#endif
#include "pmdi_sweep2_body.h"
#include "pmdi_sweep_carve.h"      // pmdi_sweep_lds_bytes (the build without the general kernel's code has not seen it yet)

namespace {

// Two waves per SIMD whatever the workgroup's width (64 * NW threads: two 256-thread workgroups per CU, or one of 512) -- the second
// launch bound is hipcc's waves-per-SIMD floor -- so a wave may use up to 256 VGPRs.  The particle state and the cluster cache of a wave live in registers for the whole sweep; the builds' spill
// counts are pinned by tests/test_build_budget.py.
template <int K, int PPL, int NW, bool GO>
__global__ void __launch_bounds__(64 * NW, 2) pmdi_sweep2_kernel(const SweepArgs *__restrict__ ap)
{
    // which chains this workgroup sweeps -- the one at its index, the one it draws, or one after the other until none is left:
    // pmdi_sweep2_body.h, sweep_slots
    pmdi_s2::sweep_slots<K, PPL, NW, GO>(ap);
}

// the instantiations: one per shape of pmdi_s2::shape_for (pmdi_sweep2_layout.h)
// (gauss_only: every dataset of the handle is Gaussian -- the build without the integer cluster types' code; 4-wave shapes only)
template <int K>
const void *kernel_for_k(int P, int *nw, bool gauss_only)
{
    const pmdi_s2::Shape s = pmdi_s2::shape_for(P);
    *nw = s.nw;
    if (s.nw == 4 && gauss_only) {
        if (s.ppl == 1) return (const void *)pmdi_sweep2_kernel<K, 1, 4, true>;
        if (s.ppl == 2) return (const void *)pmdi_sweep2_kernel<K, 2, 4, true>;
        if (s.ppl == 4) return (const void *)pmdi_sweep2_kernel<K, 4, 4, true>;
    }
    if (s.nw == 4 && s.ppl == 1) return (const void *)pmdi_sweep2_kernel<K, 1, 4, false>;
    if (s.nw == 4 && s.ppl == 2) return (const void *)pmdi_sweep2_kernel<K, 2, 4, false>;
    if (s.nw == 4 && s.ppl == 4) return (const void *)pmdi_sweep2_kernel<K, 4, 4, false>;
    if (s.nw == 8 && s.ppl == 4) return (const void *)pmdi_sweep2_kernel<K, 4, 8, false>;
    return nullptr;
}

const void *kernel_for(int K, int P, int *nw, bool gauss_only = false)
{
    switch (K) {
    case 1: return kernel_for_k<1>(P, nw, gauss_only);
    case 2: return kernel_for_k<2>(P, nw, gauss_only);
    case 3: return kernel_for_k<3>(P, nw, gauss_only);
    case 4: return kernel_for_k<4>(P, nw, gauss_only);
    }
    return nullptr;
}

bool all_gaussian(const SweepArgs &a)
{
    for (int k = 0; k < a.K; ++k) if (a.ds[k].kind != K_GAUSSIAN) return false;
    return true;
}

}  // namespace

// dynamic LDS of a launch: this kernel's layout, or the general kernel's for the same workgroup width when a handed-over chain is
// carried on in place and that layout is the larger one
static size_t launch_lds(const SweepArgs &a, int nw)
{
    size_t lds = (size_t)a.s2.total;
    if (a.resume) { const size_t g = pmdi_sweep_lds_bytes(a, 64 * nw); if (g > lds) lds = g; }
    return lds;
}

hipError_t pmdi_sweep2_blocks_per_cu(const SweepArgs &a, int *blocks)
{
    int nw = 0;
    const void *fn = kernel_for(a.K, a.P, &nw, all_gaussian(a));
    if (!fn) return hipErrorInvalidValue;
    const size_t lds = launch_lds(a, nw);
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, fn, 64 * nw, lds);
}

hipError_t pmdi_launch_sweep2(const SweepArgs &a_in, SweepArgs *d_args, int n_chains, int grid, hipStream_t stream, SweepArgs *staging)
{
    SweepArgs a = a_in;
    a.n_slots = n_chains;
    // (one-shot workgroups sweep one chain each; the position a workgroup drew is kept under 1 + its index: n_chains words)
    if (grid < 1 || grid > n_chains || (grid < n_chains && !(a.ticket && a.hold == 2))) return hipErrorInvalidValue;
    int nw = 0;
    const void *fn = kernel_for(a.K, a.P, &nw, all_gaussian(a));
    if (!fn) return hipErrorInvalidValue;
    const size_t lds = launch_lds(a, nw);
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    const SweepArgs *src = &a;
    if (staging) { *staging = a; src = staging; }
    e = hipMemcpyAsync(d_args, src, sizeof(SweepArgs), hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) return e;
    if (a.ticket) {
        e = hipMemsetAsync(a.ticket, 0, sizeof(int), stream);
        if (e != hipSuccess) return e;
    }
    const SweepArgs *ap = d_args;
    void *args[] = {(void *)&ap};
    e = hipLaunchKernel(fn, dim3((unsigned)grid), dim3(64u * (unsigned)nw), args, lds, stream);
    if (e != hipSuccess) return e;
    return hipGetLastError();
}
