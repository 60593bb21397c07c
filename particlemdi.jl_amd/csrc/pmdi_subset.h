// pmdi_subset.h -- sums over all N^K label combinations of
//     prod_k g[k][c_k] * prod_{a<b} (1 + Phi_ab [c_a == c_b])
// without the N^K table, stated once for the hyper-parameter updates (pmdi_hypers.hip) and for the coupled placement of held-out
// rows (pmdi_predict_coupled.hip).  Expanding the pair product over edge subsets E of the complete graph on the K datasets,
//     prod_{a<b} (1 + Phi_ab [c_a == c_b]) = sum_E prod_{e in E} Phi_e * [c constant on every component of E],
// and grouping the subsets by the partition of {1..K} their components induce, every such sum becomes a sum over set partitions
// of products of
//     T(B)    = sum_m prod_{j in B} g[j][m]                  (one label shared by the datasets of block B)
//     conn(B) = sum over connected spanning edge sets of B of prod Phi_e,
// i.e. Z = sum_{partitions pi} prod_{B in pi} conn(B) T(B), evaluated by a subset recursion (Zs below), and
//     sum_{c : c_k = m} (...)   = sum_{B containing k} conn(B) prod_{j in B} g[j][m] * Zs(complement of B)
//     sum_{c : c_a = c_b} (...) = (1 + Phi_ab) * the same sum with a and b contracted into one vertex.
// conn(B) is built from positive terms only (no inclusion-exclusion differences): remove the lowest vertex v of B; the rest
// falls into connected pieces C_i, each tied to v by a non-empty edge set:
//     conn(B) = sum_{partitions {C_i} of B - v} prod_i conn(C_i) * (prod_{u in C_i} (1 + Phi_vu) - 1).
// K <= 8: masks < 256, W is the symmetric 8 x 8 pair-weight matrix.  Every function is one lane's work in a fixed order of
// operations; which lane runs it changes no result.  Compile with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

namespace pmdi_dev {

// conn[B] for every non-empty B inside `active`; F and link are scratch of 256 doubles each
__device__ inline void conn_all(unsigned active, const double *W, double *conn, double *F, double *link)
{
    unsigned B = 0;
    while ((B = (B - active) & active) != 0) {
        const int v = __ffs((int)B) - 1;
        const unsigned R = B & (B - 1);
        if (R == 0) { conn[B] = 1.0; continue; }
        link[0] = 0.0;
        unsigned C = 0;
        while ((C = (C - R) & R) != 0) {                       // prod_{u in C} (1 + W[v][u]) - 1, positive terms only
            const int hb = 31 - __clz((int)C);
            const double w = W[v * 8 + hb], r = link[C ^ (1u << hb)];
            link[C] = r + w + r * w;
        }
        F[0] = 1.0;
        unsigned S = 0;
        while ((S = (S - R) & R) != 0) {
            const unsigned l = S & (0u - S), Sp = S ^ l;
            double acc = 0.0;
            unsigned Cp = 0;
            do {
                const unsigned Cc = Cp | l;
                acc += conn[Cc] * link[Cc] * F[Sp ^ Cp];
                Cp = (Cp - Sp) & Sp;
            } while (Cp != 0);
            F[S] = acc;
        }
        conn[B] = F[R];
    }
}

// Zs[S] for one non-empty S, from the Zs of its proper subsets: the block of S's lowest member runs over the subsets that hold it
__device__ __forceinline__ double zs_one(unsigned S, const double *conn, const double *T, const double *Zs)
{
    const unsigned l = S & (0u - S), Sp = S ^ l;
    double acc = 0.0;
    unsigned Cp = 0;
    do {
        const unsigned B = Cp | l;
        acc += conn[B] * T[B] * Zs[Sp ^ Cp];
        Cp = (Cp - Sp) & Sp;
    } while (Cp != 0);
    return acc;
}

// Zs[S] = sum over set partitions of S of prod conn(B) T(B), for every S inside `active`
__device__ inline void zs_all(unsigned active, const double *conn, const double *T, double *Zs)
{
    Zs[0] = 1.0;
    unsigned S = 0;
    while ((S = (S - active) & active) != 0) Zs[S] = zs_one(S, conn, T, Zs);
}

// W from the pair weights in Phi's own order: (0,1), (0,2), ..., (K-2,K-1)
__device__ __forceinline__ void fill_W(int K, const double *Phi, double *W)
{
    int i = 0;
    for (int a = 0; a < K - 1; ++a)
        for (int b = a + 1; b < K; ++b) { W[a * 8 + b] = Phi[i]; W[b * 8 + a] = Phi[i]; ++i; }
}

// T[B] for one non-empty B: labels ascending, the product over the datasets ascending
__device__ __forceinline__ double T_one(int K, int N, unsigned B, const double *ge)
{
    double acc = 0.0;
    for (int m = 0; m < N; ++m) {
        double p = 1.0;
        for (int j = 0; j < K; ++j) if (B & (1u << j)) p = p * ge[j * N + m];
        acc += p;
    }
    return acc;
}

// T[B] = sum_m prod_{j in B} ge[j][m] for every non-empty B (lanes = subsets)
__device__ __forceinline__ void compute_T(int K, int N, const double *ge, double *T, int tid, int nthreads)
{
    for (unsigned B = 1 + tid; B < (1u << K); B += nthreads) T[B] = T_one(K, N, B, ge);
}

// The sum over the label combinations whose k-th label is m; U = the other datasets, Zs holds every subset of U
__device__ __forceinline__ double marginal_sum(int K, int N, int k, int m, unsigned U, const double *conn, const double *ge, const double *Zs)
{
    double S = 0.0;
    unsigned Cq = 0;
    do {
        const unsigned B = Cq | (1u << k);
        double p = 1.0;
        for (int j = 0; j < K; ++j) if (B & (1u << j)) p = p * ge[j * N + m];
        S += conn[B] * p * Zs[U ^ Cq];
        Cq = (Cq - U) & U;
    } while (Cq != 0);
    return S;
}

// Contract b into a: the merged vertex keeps index a; its weight to u is (1 + W_au)(1 + W_bu) - 1
__device__ __forceinline__ void contract_W(int K, int ka, int kb, const double *W, double *W2)
{
    for (int e = 0; e < 64; ++e) W2[e] = W[e];
    for (int u = 0; u < K; ++u) {
        if (u == ka || u == kb) continue;
        const double wa = W[ka * 8 + u], wb = W[kb * 8 + u];
        const double w = wa + wb + wa * wb;
        W2[ka * 8 + u] = w; W2[u * 8 + ka] = w;
    }
}

// The sum over the label combinations with c_a == c_b, before its factor (1 + Phi_ab); conn2 = conn_all(full - b, W2),
// rest = the datasets other than a and b, Zs holds every subset of rest
__device__ __forceinline__ double pair_sum(int ka, int kb, unsigned rest, const double *conn2, const double *T, const double *Zs)
{
    double S = 0.0;
    unsigned Cq = 0;
    do {
        S += conn2[Cq | (1u << ka)] * T[Cq | (1u << ka) | (1u << kb)] * Zs[rest ^ Cq];
        Cq = (Cq - rest) & rest;
    } while (Cq != 0);
    return S;
}

}  // namespace pmdi_dev
