"""The yardstick of the density accumulator (include/pmdi_hip.h, pmdi_density_*): a plain Python mirror of one add, float loops in
the stated order with the C library's log, lgamma and exp, and the replay of the accumulator's state from per-add values.  Z comes
from the subset recursion restated in tests/_np_predict_coupled.py; z_enumerated sums all N^K label tuples to hold it to.
TEST INFRASTRUCTURE ONLY."""
import itertools
import math

import numpy as np

from _np_loo import cexp, clgamma, clog
from _np_predict import same_bits, ulps  # noqa: F401  (shared helpers of the mirrors)
from _np_predict_coupled import compute_T, conn_all, fill_W, pairs, zs_all

Q_ONE = 1 << 20
INF_I = 0x7FFFFFFF


def gauss_lm_table(m):
    """LM[m] of pmdi_create: gaussian_cluster.jl:76-79, the part that depends on the cluster's size only."""
    nn = float(m)
    a_n, a_0, b_0, k_0 = nn / 2.0 + 0.5, 0.5, 0.5, 0.001
    k_n = nn + k_0
    return (a_0 * clog(b_0)) + clgamma(a_n) - clgamma(a_0) + 0.5 * (clog(k_0) - clog(k_n)) - (nn * 0.5) * clog(2.0 * math.pi)


def label_lm(x, kind, members):
    """calc_logmarginal per feature of the cluster of `members` (ascending rows) with every feature on: a list of D floats."""
    n_rows, D = x.shape
    cn = len(members)
    out = []
    for q in range(D):
        if kind == "gaussian":
            sg, bt = 0.0, 0.5
            for j, i in enumerate(members):          # pmdi_arith::gauss_add_sb
                nnew = j + 1
                mu_prev = 0.0 if nnew == 1 else sg / ((nnew - 1) + 0.001)
                xv = float(x[i, q])
                sg = sg + xv
                d = xv - mu_prev
                bt = bt + ((nnew - 1) + 0.001) * (d * d) / (2.0 * (nnew + 0.001))
            a_n = cn / 2.0 + 0.5
            out.append((-a_n) * clog(bt) + gauss_lm_table(cn))
        elif kind == "categorical":
            mc = int(x[:, q].max())
            counts = [0] * mc
            for i in members:
                counts[int(x[i, q]) - 1] += 1
            v = 0.0
            v += clgamma(0.5 * (2 * mc)) - clgamma(0.5 * (2 * (mc + cn)))
            for r in range(mc):
                v += clgamma(0.5 * (2 * counts[r] + 1))
            out.append(v)
        else:
            S = sum(int(x[i, q]) for i in members)
            out.append(clgamma(float(S + 1)) - clgamma(float(S + (cn + 1 + 1))) + clgamma(float(1 + cn)))
    return out


def fnull(train, kinds):
    """[sumD]: -(log marginal of the one-cluster allocation), what pmdi_create keeps."""
    out = []
    for x, kind in zip(train, kinds):
        out += [-v for v in label_lm(x, kind, list(range(x.shape[0])))]
    return np.array(out)


def counts_first(s_row, N):
    """cn[l], first[l] of one (chain, dataset); a label outside 0..N-1 is a member of nothing."""
    cn, first = np.zeros(N, dtype=np.int64), np.full(N, INF_I, dtype=np.int64)
    for i, v in enumerate(s_row):
        if 0 <= v < N:
            cn[v] += 1
            first[v] = min(first[v], i)
    return cn, first


def feature_terms(fn, lm, first):
    """Step 3 for one (chain, dataset): fn (D,), lm (D, N), first (N,) -> bf (D,), cl (D,), float loops."""
    order = [l for l in np.argsort(first, kind="stable") if first[l] != INF_I]
    bf, cl = [], []
    for q in range(len(fn)):
        b, c = float(fn[q]) + 0.0, 0.0
        for l in order:
            b += float(lm[q][l])
            c += float(lm[q][l])
        bf.append(b)
        cl.append(c)
    return np.array(bf), np.array(cl)


def q_of(bf):
    if not math.isfinite(bf):
        return 0
    pr = 1.0 - 1.0 / cexp(bf + 1.0)
    return int(math.floor(pr * 1048576.0 + 0.5)) if pr > 0.0 else 0


def dataset_ll(cl, fn, fl):
    """Step 4: ((t_0 + t_1) + ...), t_q = flag ? cl : -fnull."""
    ll = None
    for q in range(len(cl)):
        t = float(cl[q]) if (fl is None or fl[q]) else -float(fn[q])
        ll = t if ll is None else ll + t
    return ll


def z_recursion(K, N, Pi, Phi):
    full = (1 << K) - 1
    W = fill_W(K, Phi if K > 1 else [])
    conn = conn_all(full, W)
    T = compute_T(K, N, [[float(v) for v in row] for row in Pi])
    return zs_all(full, conn, T)[full]


def z_enumerated(K, N, Pi, Phi):
    """The sum over all N^K label tuples, term by term (math.fsum: the yardstick of the recursion)."""
    terms = []
    for c in itertools.product(range(N), repeat=K):
        p = 1.0
        for k in range(K):
            p *= float(Pi[k][c[k]])
        for i, (a, b) in enumerate(pairs(K)):
            if c[a] == c[b]:
                p *= 1.0 + float(Phi[i])
        terms.append(p)
    return math.fsum(terms)


def agree_counts(s_chain):
    K = s_chain.shape[0]
    return np.array([int((s_chain[a] == s_chain[b]).sum()) for a, b in pairs(K)] or [0], dtype=np.int64)


def log_prior(cn, Pi, agree, Phi, n, logZ):
    """Step 5 from cn (K, N), Pi (K, N), agree (G,), Phi (G,) and log Z."""
    K, N = cn.shape
    lp = 0.0
    for k in range(K):
        for l in range(N):
            if cn[k, l] > 0:
                lp += float(cn[k, l]) * clog(float(Pi[k, l]))
    for p in range(K * (K - 1) // 2):
        lp += float(agree[p]) * clog(1.0 + float(Phi[p]))
    lp -= float(n) * logZ
    return lp


def log_joint(ll, lprior):
    lj = float(ll[0])
    for k in range(1, len(ll)):
        lj = lj + float(ll[k])
    return lj + lprior


def one_add(train, kinds, s, Pi, Phi, flags, N):
    """The whole add: s (C, K, n) 0-based, Pi (C, K, N), Phi (C, max(1, G)), flags (C, sumD) or None.  Returns a dict of the
    arrays pmdi_density_last gives plus ll (C, K), lprior (C,), lj (C,)."""
    C_, K, n = s.shape
    D = [x.shape[1] for x in train]
    offs = np.concatenate([[0], np.cumsum(D)])
    sumD = int(offs[-1])
    fn = fnull(train, kinds)
    out = {"cn": np.zeros((C_, K, N), dtype=np.int64), "first": np.zeros((C_, K, N), dtype=np.int64), "lm": np.zeros((C_, sumD, N)),
           "bf": np.zeros((C_, sumD)), "cl": np.zeros((C_, sumD)), "q": np.zeros((C_, sumD), dtype=np.int64),
           "agree": np.zeros((C_, max(1, K * (K - 1) // 2)), dtype=np.int64), "logZ": np.zeros(C_),
           "ll": np.zeros((C_, K)), "lprior": np.zeros(C_), "lj": np.zeros(C_)}
    for c in range(C_):
        for k in range(K):
            cn, first = counts_first(s[c, k], N)
            out["cn"][c, k], out["first"][c, k] = cn, first
            g0, g1 = int(offs[k]), int(offs[k + 1])
            for l in range(N):
                if cn[l] > 0:
                    out["lm"][c, g0:g1, l] = label_lm(train[k], kinds[k], [int(i) for i in np.flatnonzero(s[c, k] == l)])
            bf, cl = feature_terms(fn[g0:g1], out["lm"][c, g0:g1], first)
            out["bf"][c, g0:g1], out["cl"][c, g0:g1] = bf, cl
            out["q"][c, g0:g1] = [q_of(float(v)) for v in bf]
            out["ll"][c, k] = dataset_ll(cl, fn[g0:g1], None if flags is None else flags[c, g0:g1])
        if K > 1:
            out["agree"][c] = agree_counts(s[c])
        out["logZ"][c] = clog(z_recursion(K, N, Pi[c], Phi[c]))
        out["lprior"][c] = log_prior(out["cn"][c], Pi[c], out["agree"][c], Phi[c], n, out["logZ"][c])
        out["lj"][c] = log_joint(out["ll"][c], out["lprior"][c])
    return out


class Mirror:
    """The accumulator's state replayed from per-add values: the traces, the best state per chain, the four feature sums."""

    def __init__(self, C_, K, n, sumD):
        self.C, self.K, self.n, self.sumD = C_, K, n, sumD
        self.reset()

    def reset(self):
        self.T = 0
        self.best_val = np.full(self.C, -np.inf)
        self.best_t = np.full(self.C, -1, dtype=np.int64)
        self.best_s = np.zeros((self.C, self.K, self.n), dtype=np.uint8)
        self.bf_sum, self.bf_sq_sum = np.zeros(self.sumD), np.zeros(self.sumD)
        self.p_sum, self.bad = np.zeros(self.sumD, dtype=np.int64), np.zeros(self.sumD, dtype=np.int64)

    def add(self, lj, s, bf, q):
        """lj (C,), s (C, K, n), bf (C, sumD), q (C, sumD): one add's values (the device's own, or the mirror's)."""
        for c in range(self.C):
            if float(lj[c]) > float(self.best_val[c]):      # a tie keeps the earlier state; a NaN never wins
                self.best_val[c], self.best_t[c], self.best_s[c] = lj[c], self.T, s[c]
        for g in range(self.sumD):
            s1, s2 = float(self.bf_sum[g]), float(self.bf_sq_sum[g])
            for c in range(self.C):
                v = float(bf[c, g])
                if not math.isfinite(v):
                    self.bad[g] += 1
                    continue
                s1 += v
                s2 += v * v
                self.p_sum[g] += int(q[c, g])
            self.bf_sum[g], self.bf_sq_sum[g] = s1, s2
        self.T += 1

    def arrays(self):
        return {"best_val": self.best_val, "best_t": self.best_t, "best_s": self.best_s, "bf_sum": self.bf_sum,
                "bf_sq_sum": self.bf_sq_sum, "p_sum": self.p_sum, "bad": self.bad}
