// emu_sweep_slots.cpp -- TEST INFRASTRUCTURE ONLY.  The entry loop of the settled-chain kernel (pmdi_s2::sweep_slots of
// particlemdi.jl_amd/csrc/pmdi_sweep2_body.h) on the host: ONE emulated workgroup keeps its slot and sweeps several chains back to
// back, drawing each from the ticket.  Before every chain the whole LDS is filled with a non-zero byte pattern, so a sweep that relies
// on what the LDS held before it -- zeros of a fresh process, or the previous chain's tables -- gives different results here.
// Everything else (the data, the host-built tables, the arena layout) is emu_sweep2.cpp's, compiled into this translation unit.
#include <cstring>

#include "lane_api_emu.h"

namespace emu_slots {
size_t g_lds_bytes = 0;
int g_poisoned = 0;         // chains taken up so far (every one found a poisoned LDS)
constexpr unsigned char LDS_BYTE = 0xA5;
inline void poison_lds()
{
    if (PM2_TID() == 0) { memset(PM2_SMEM, LDS_BYTE, g_lds_bytes); ++g_poisoned; }
    PM2_BARRIER();
}
}  // namespace emu_slots
#define PM2_SLOT_HOOK() emu_slots::poison_lds()

#include "emu_sweep2.cpp"

namespace {

template <int K, int PPL> void slots_body(const SweepArgs *a, bool gauss_only)
{
    if (gauss_only) pmdi_s2::sweep_slots<K, PPL, 4, true>(a);
    else pmdi_s2::sweep_slots<K, PPL, 4, false>(a);
}

// (two datasets, 256 particles: the shape tests/test_emu_sweep_slots.py runs -- every further build costs the suite compile time)
void slots_entry(void *p)
{
    const RunArg *r = (const RunArg *)p;
    if (r->K == 2 && r->NW == 4 && r->PPL == 1) return slots_body<2, 1>(r->a, r->gauss_only);
    fprintf(stderr, "emu slots: unsupported K=%d PPL=%d NW=%d\n", r->K, r->PPL, r->NW);
    abort();
}

}  // namespace

extern "C" {

// 1 if emu_sweep_slots has a build for the handle's shape
int emu_slots_supported(void *h)
{
    const Emu *e = (const Emu *)h;
    const pmdi_s2::Shape s = pmdi_s2::shape_for(e->K, e->P);
    return e->K == 2 && s.nw == 4 && s.ppl == 1;
}

// C chains of the handle's model, chain c with seed + c (as the device numbers them), swept by ONE workgroup through the entry loop
// (hold = 2, a launch of one workgroup).  Inputs and outputs per chain, chain-major, as the device holds them: s_in / s_out [C][K][n]
// 0-based, order [C][n], Pi [C][K][N], logphi [C][npairs], lw_out [C][P], pstar [C], stats [C][8], work [C][K][8], err [C],
// swept_by [C] (1: the settled-chain kernel finished the chain), particle [C][K][P][N], counts / cn [C][K][cap], maxid [C][K].
// Returns the number of chains that found a poisoned LDS (C when all went well), or EMU_E_GUARD.
int emu_sweep_slots(void *h, int C, long long iter, const int *s_in, const int *order, long long n1, const double *Pi, const double *logphi,
                    double lw_init, int *s_out, double *lw_out, int *pstar, long long *stats, long long *work, int *err, int *swept_by,
                    int *particle, int *counts, int *cn, int *maxid_out)
{
    Emu *e = (Emu *)h;
    SweepArgs a;
    memset(&a, 0, sizeof(a));
    a.K = e->K; a.N = e->N; a.P = e->P; a.cap = (int)e->cap;
    a.Dmax = e->Dmax; a.sumD = e->sumD; a.npairs = e->K > 1 ? e->K * (e->K - 1) / 2 : 1;
    a.q1 = e->q1; a.q2 = 0;
    a.iter = (unsigned)iter; a.n = e->n; a.n1 = n1; a.seed = e->seed; a.lw_init = lw_init;
    // the chains' arenas side by side, as on the device, between two guard regions
    std::vector<std::vector<char>> arena(e->K);
    for (int k = 0; k < e->K; ++k) {
        a.ds[k] = e->ds[k];
        const size_t stride = a.ds[k].stride;
        arena[k].assign(GUARD + stride * C + GUARD, 0);
        memset(arena[k].data(), GUARD_BYTE, GUARD);
        memset(arena[k].data() + GUARD + stride * C, GUARD_BYTE, GUARD);
        a.ds[k].arena = arena[k].data() + GUARD;
    }
    a.s_in = s_in; a.order = order; a.Pi = Pi; a.logphi = logphi;
    a.s_out = s_out; a.lw_out = lw_out; a.pstar = pstar; a.stats = stats; a.err = err; a.swept_by = swept_by;
    std::vector<long long> cost(C, 0), wk((size_t)C * PMDI_KMAX_I * 8, 0);
    std::vector<int> kstate((size_t)C * PMDI_KMAX_I * 2, 0);
    a.cost = cost.data(); a.kstate = kstate.data(); a.work = wk.data();
    // one workgroup, its position in the launch order drawn anew for every chain
    std::vector<int> ticket(2, 0);
    a.ticket = ticket.data(); a.hold = 2; a.n_slots = C;
    pmdi_s2::make_layout(e->K, e->N, e->P, e->Dmax, e->cols_l, e->idcap, e->cls, e->cdfl, a.s2);
    const pmdi_s2::Shape shape = pmdi_s2::shape_for(e->K, e->P);
    bool go = true;
    for (int k = 0; k < e->K; ++k) go = go && e->ds[k].kind == K_GAUSSIAN;
    RunArg r{&a, e->K, shape.ppl, shape.nw, go};
    emu_slots::g_lds_bytes = (size_t)a.s2.total;
    emu_slots::g_poisoned = 0;
    wavesim::run_block(64 * shape.nw, 0, (size_t)a.s2.total, slots_entry, &r);
    for (int k = 0; k < e->K; ++k) {
        const unsigned char *g = (const unsigned char *)arena[k].data();
        const size_t len = a.ds[k].stride * C;
        for (size_t j = 0; j < GUARD; ++j)
            if (g[j] != GUARD_BYTE || g[GUARD + len + j] != GUARD_BYTE) {
                fprintf(stderr, "emu slots: dataset %d: a guard byte around the %d arenas was written\n", k, C);
                return EMU_E_GUARD;
            }
    }
    if (ticket[0] != C + 1) { fprintf(stderr, "emu slots: %d draws for %d chains\n", ticket[0], C); return -1; }
    for (int c = 0; c < C; ++c)
        for (int k = 0; k < e->K; ++k) {
            for (int j = 0; j < 8; ++j) work[((size_t)c * e->K + k) * 8 + j] = wk[((size_t)c * PMDI_KMAX_I + k) * 8 + j];
            if (err[c] != 0) continue;
            // what pmdi_export_state does: expand the columns back to particle[n, p, k]
            const DsetDev &d = a.ds[k];
            const char *ar = d.arena + (size_t)c * d.stride;
            const int *tab = (const int *)(ar + d.o_particle[0]);
            const int *col = (const int *)(ar + d.o_col);
            for (int p = 0; p < e->P; ++p)
                for (int nn = 0; nn < e->N; ++nn)
                    particle[(((size_t)c * e->K + k) * e->P + p) * e->N + nn] = tab[(size_t)col[p] * e->N + nn];
            const int *cc = (const int *)(ar + d.o_counts), *cnn = (const int *)(ar + d.o_cn);
            for (long long id = 1; id <= e->cap; ++id) {
                counts[((size_t)c * e->K + k) * e->cap + (id - 1)] = cc[id];
                cn[((size_t)c * e->K + k) * e->cap + (id - 1)] = cnn[id];
            }
            maxid_out[c * e->K + k] = kstate[((size_t)c * PMDI_KMAX_I + k) * 2];
        }
    return emu_slots::g_poisoned;
}

}  // extern "C"
