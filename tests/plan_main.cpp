// Stand-alone driver of the launch planner (csrc/pmdi_plan.cpp): reads cases from stdin, one per line -- the integers of a row of
// tests/_plan_cases.py FIELDS, then the device's CU count, whether stream wait-value is usable, and the workgroups per CU the
// occupancy callback answers -- and prints per case: the return code, the 32 words of pmdi_plan_layout32, the LDS bytes of the wide
// layout, and the error text.  Built and run by tests/test_plan_host.py with -fsanitize=address,undefined; no GPU, no HIP call.
#include <cstdarg>
#include <cstdio>
#include <sstream>
#include <string>
#include <vector>

#include "pmdi_plan.h"
#include "pmdi_sweep_carve.h"

static char g_err[512];
static int g_asked;         // times the occupancy callback was consulted for the current case

int pmdi_set_error(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int main()
{
    enum { F_K, F_N, F_P, F_n, F_CHAINS, F_Q1, F_Q2, F_BLOCK, F_CAP, F_D0, F_KIND0 = F_D0 + 8, F_KNOB0 = F_KIND0 + 8,
           F_CUS = F_KNOB0 + 19, F_WAIT, F_OCC, F_COUNT };
    static_assert(sizeof(pmdi_tuning) == 24 * sizeof(int32_t), "19 knobs and 5 reserved words");
    char line[4096];
    while (fgets(line, sizeof(line), stdin)) {
        std::istringstream in(line);
        std::vector<long long> v;
        for (long long x; in >> x;) v.push_back(x);
        if (v.empty()) continue;
        if ((int)v.size() != F_COUNT) { fprintf(stderr, "a case has %d fields, not %zu\n", (int)F_COUNT, v.size()); return 2; }
        pmdi_config cfg{};
        cfg.abi_version = PMDI_ABI_VERSION;
        cfg.K = (int)v[F_K]; cfg.N = (int)v[F_N]; cfg.P = (int)v[F_P]; cfg.n = v[F_n]; cfg.n_chains = (int)v[F_CHAINS];
        cfg.q1_mode = (int)v[F_Q1]; cfg.q2_mode = (int)v[F_Q2]; cfg.block_threads = (int)v[F_BLOCK]; cfg.pool_cap = v[F_CAP];
        pmdi_tuning tn;
        for (int i = 0; i < 24; ++i) ((int32_t *)&tn)[i] = i < 19 ? (int32_t)v[F_KNOB0 + i] : -1;
        int Dmax = 0;
        for (int k = 0; k < cfg.K && k < 8; ++k) if (v[F_D0 + k] > Dmax) Dmax = (int)v[F_D0 + k];
        long long cap = cfg.pool_cap > 0 ? cfg.pool_cap : (long long)cfg.N * cfg.P + 1;      // as pmdi_create
        if (cap > (long long)cfg.N * cfg.P + 1) cap = (long long)cfg.N * cfg.P + 1;
        PlanDevice dev;
        dev.cus = (int)v[F_CUS]; dev.wait_value = v[F_WAIT] != 0;
        const int occ = (int)v[F_OCC];
        g_asked = 0;
        dev.blocks_per_cu = [occ](const SweepArgs &, int) { ++g_asked; return occ; };
        SweepPlan plan;
        g_err[0] = 0;
        const int rc = pmdi_plan_sweep(cfg, tn, Dmax, cap, dev, &plan);
        int32_t w[32] = {0};
        long long lds = 0;
        if (rc == PMDI_OK) {
            pmdi_plan_layout32(plan, plan.want_gate, plan.want_xchg, cfg.K, cfg.P, w);
            SweepArgs a{};
            a.K = cfg.K; a.N = cfg.N; a.P = cfg.P; a.Dmax = Dmax; a.item_cap = cfg.N > 32 ? PMDI_ITEM_CAP_BIGN : PMDI_ITEM_CAP;
            a.ksplit = plan.ksplit;
            pmdi_put_tables(plan.wide, a);
            lds = (long long)pmdi_sweep_lds_bytes(a, plan.T);
            g_err[0] = 0;       // (a light or hand-over layout that did not fit is no error of the plan)
        }
        printf("%d", rc);
        for (int i = 0; i < 32; ++i) printf(" %d", w[i]);
        printf(" %lld %d |%s\n", lds, g_asked, g_err);
    }
    return 0;
}
