// arith_main.cpp -- TEST INFRASTRUCTURE ONLY.  A stand-alone host program around particlemdi.jl_amd/csrc/pmdi_arith.h, built by
// tests/test_arith_host.py with the host compiler (-ffp-contract=off, address and undefined-behaviour sanitizers) and run as a
// program: it reads cases from standard input and prints every double as the 16 hex digits of its bits.
//   arith_main uniform    lines "seed iter pos k p site" (seed decimal, 64 bits)   -> uniform01
//   arith_main resample   lines "u01-bits P"                                       -> resample_u_at(u01, P, j) for every j < P
//   arith_main gauss      lines "x-bits": a chain of adds from the empty cluster    -> per step: the two terms of calc_logprob for
//                         x before the add, then Sigma, beta (gauss_add_sb), mu, lambda (gauss_ml), and mu, lambda, Sigma, beta
//                         of the full gauss_add
//   arith_main ess        lines "ess-bits P"                                       -> ess_needs_sequential_redo, ess_resamples
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../particlemdi.jl_amd/csrc/pmdi_arith.h"

static unsigned long long bits(double v) { unsigned long long u; memcpy(&u, &v, 8); return u; }
static double from_bits(unsigned long long u) { double v; memcpy(&v, &u, 8); return v; }

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    const char *mode = argv[1];
    if (!strcmp(mode, "uniform")) {
        unsigned long long seed;
        unsigned iter, pos, k, p, site;
        while (scanf("%llu %u %u %u %u %u", &seed, &iter, &pos, &k, &p, &site) == 6)
            printf("%016llx\n", bits(pmdi_arith::uniform01(seed, iter, pos, k, p, site)));
    } else if (!strcmp(mode, "resample")) {
        unsigned long long ub;
        int P;
        while (scanf("%llx %d", &ub, &P) == 2)
            for (int j = 0; j < P; ++j) printf("%016llx\n", bits(pmdi_arith::resample_u_at(from_bits(ub), P, j)));
    } else if (!strcmp(mode, "gauss")) {
        double sg = 0.0, bt = 0.5;                        // the empty cluster (gaussian_cluster.jl: Sigma = 0, beta = 0.5)
        double mu4 = 0.0, lam4 = 1.0, sg4 = 0.0, bt4 = 0.5;
        int n = 0;
        unsigned long long xb;
        while (scanf("%llx", &xb) == 1) {
            const double x = from_bits(xb);
            double mu, lam, ta, tb;
            pmdi_arith::gauss_ml(n, sg, bt, mu, lam);
            pmdi_arith::gauss_terms(x, (double)n, mu, lam, ta, tb);
            ++n;
            pmdi_arith::gauss_add_sb(x, n, sg, bt);
            pmdi_arith::gauss_ml(n, sg, bt, mu, lam);
            pmdi_arith::gauss_add(x, n, mu4, lam4, sg4, bt4);
            printf("%016llx %016llx %016llx %016llx %016llx %016llx %016llx %016llx %016llx %016llx\n", bits(ta), bits(tb), bits(sg),
                   bits(bt), bits(mu), bits(lam), bits(mu4), bits(lam4), bits(sg4), bits(bt4));
        }
    } else if (!strcmp(mode, "ess")) {
        unsigned long long eb;
        int P;
        while (scanf("%llx %d", &eb, &P) == 2)
            printf("%d %d\n", (int)pmdi_arith::ess_needs_sequential_redo(from_bits(eb), P), (int)pmdi_arith::ess_resamples(from_bits(eb), P));
    } else {
        return 2;
    }
    return 0;
}
