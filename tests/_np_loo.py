"""The yardstick of the leave-one-out accumulator (include/pmdi_hip.h, pmdi_loo_*): a plain Python mirror of one add.  Clusters are
built by the CPU oracle's cluster_add! in ascending row order under the chain's flags and evaluated by its calc_logprob.  The row's
own label comes in two forms: (a) "downdate", the stated downdate of the full cluster's statistics (oracle Cluster.stats), evaluated
by calc_logprob restated here on Python floats with the C library's log and lgamma; (b) "rebuild", an oracle cluster of the members
without the row.  Weights and fixed point are Python float loops, the pair (E, S) exact Python integers, the sums float and integer loops.  TEST INFRASTRUCTURE ONLY."""
import ctypes
import ctypes.util
import math

import numpy as np

from _np_predict import same_bits, split_flags, ulps  # noqa: F401  (shared helpers of the two mirrors)

Q_ONE = 1 << 20
E_EMPTY = -9187201950435737472
LOG2E = 1.4426950408889634

_m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _f in ("log", "lgamma", "exp2", "exp"):
    getattr(_m, _f).restype = ctypes.c_double
    getattr(_m, _f).argtypes = [ctypes.c_double]
clog, clgamma, cexp2, cexp = _m.log, _m.lgamma, _m.exp2, _m.exp      # the oracle's libm, not CPython's own lgamma


def gauss_remove_sb(x, cn, sg, bt):
    """pmdi_arith::gauss_remove_sb, operation by operation."""
    if cn == 1:
        return 0.0, 0.5
    sg = sg - x
    mu = sg / ((cn - 1) + 0.001)
    d = x - mu
    bt = bt - ((cn - 1) + 0.001) * (d * d) / (2.0 * (cn + 0.001))
    return sg, (bt if bt > 0.5 else 0.5)


def gauss_ml(cn, sg, bt):
    if cn == 0:
        return 0.0, 1.0
    n = float(cn)
    return sg / (n + 0.001), ((0.5 * n + 0.5) * (n + 0.001)) / (bt * (n + 1.001))


def gauss_logprob(x, cn, sg, bt, fl):
    """calc_logprob(::GaussianCluster) of row values x against (Sigma, beta) per feature of a cluster of size cn."""
    n = float(cn)
    on = [q for q in range(len(x)) if fl is None or fl[q]]
    out = float(len(on)) * ((clog(1.0 / math.sqrt(math.pi)) + clgamma(0.5 * n + 1.0)) - clgamma(0.5 * n + 0.5))
    for q in on:
        mu, lam = gauss_ml(cn, float(sg[q]), float(bt[q]))
        out += 0.5 * clog(lam / (n + 1.0))
        d = float(x[q]) - mu
        out -= (0.5 * n + 1.0) * clog(1.0 + (1.0 / (n + 1.0)) * (d * d) * lam)
    return out


def cat_logprob(x, cn, counts, nlevels, fl):
    """calc_logprob(::CategoricalCluster): counts (L, D) of a cluster of size cn."""
    on = [q for q in range(len(x)) if fl is None or fl[q]]
    acc = 0.0
    for q in on:
        acc += clog(nlevels[q] + float(cn))
    out = -acc
    for q in on:
        out += clog(0.5) if cn == 0 else clog(0.5 + float(counts[int(x[q]) - 1, q]))
    return out


def negbin_logprob(x, cn, S, fl):
    out = 0.0
    for q in range(len(x)):
        if fl is not None and not fl[q]:
            continue
        xo, s = int(x[q]), int(S[q])
        out += clgamma(float(1 + cn + 1)) + clgamma(float(1 + xo + s)) + clgamma(float(1 + cn + 1 + s)) - \
            clgamma(float(1 + cn + 1 + 1 + xo + s)) - clgamma(float(1 + cn)) - clgamma(float(1 + s))
    return out


def own_downdate(cl, kind, x, cn, fl, nlevels=None):
    """Form (a): lp of row values x against the full cluster `cl` (oracle Cluster of size cn that holds the row) without the row.
    Returns (lp, aux); aux for Gaussian: (beta, beta') per feature that is on."""
    st = cl.stats()
    if kind == "gaussian":
        sg, bt, aux = [], [], []
        for q in range(len(x)):
            if fl is not None and not fl[q]:
                sg.append(0.0), bt.append(0.5)
                continue
            s1, b1 = gauss_remove_sb(float(x[q]), cn, float(st["Sigma"][q]), float(st["beta"][q]))
            sg.append(s1), bt.append(b1), aux.append((float(st["beta"][q]), b1))
        return gauss_logprob(x, cn - 1, sg, bt, fl), aux
    if kind == "categorical":
        counts = st["counts"].copy()
        for q in range(len(x)):
            if fl is None or fl[q]:
                counts[int(x[q]) - 1, q] -= 1
        return cat_logprob(x, cn - 1, counts, nlevels, fl), None
    S = [int(st["Sigma"][q]) - (int(x[q]) if fl is None or fl[q] else 0) for q in range(len(x))]
    return negbin_logprob(x, cn - 1, S, fl), None


def log_predictives(O, train, kinds, s, flags, N, own="rebuild"):
    """lp (C, K, n, N), cn (C, K, N), and per (c, k, i) the Gaussian (beta, beta') pairs of the downdate (own="downdate") or None.
    s (C, K, n) 0-based labels (one outside 0..N-1 is no cluster's member and no row's own label); flags (C, sumD) or None.
    own: "rebuild", "downdate", or a dict kind -> one of the two."""
    C_, K, n = s.shape
    D = [x.shape[1] for x in train]
    lp = np.zeros((C_, K, n, N))
    cnv = np.zeros((C_, K, N), dtype=np.int64)
    aux = {}
    for c in range(C_):
        fl = split_flags(None if flags is None else flags[c], D)
        for k in range(K):
            x, kind = train[k], kinds[k]
            nlev = [float(v) / 2.0 for v in x.max(axis=0)] if kind == "categorical" else None
            prior = O.Cluster(x, kind)
            e_col = np.array([prior.logprob(i, fl[k]) for i in range(n)])
            for l in range(N):
                members = np.flatnonzero(s[c, k] == l)      # ascending
                cnv[c, k, l] = members.size
                if members.size == 0:
                    lp[c, k, :, l] = e_col
                    continue
                cl = O.Cluster(x, kind)
                for i in members:
                    cl.add(int(i), fl[k])
                for i in range(n):
                    if s[c, k, i] != l:
                        lp[c, k, i, l] = cl.logprob(i, fl[k])
                    elif (own[kind] if isinstance(own, dict) else own) == "downdate":
                        lp[c, k, i, l], aux[(c, k, i)] = own_downdate(cl, kind, x[i], members.size, fl[k], nlev)
                    else:
                        rest = O.Cluster(x, kind)
                        for j in members:
                            if j != i:
                                rest.add(int(j), fl[k])
                        lp[c, k, i, l] = rest.logprob(i, fl[k])
    return lp, cnv, aux


def weight_u(s, Phi, c, k, i, l):
    """u[l] of step 3; Phi (C, G) in pair order (0,1), (0,2), ..., or None."""
    u = 1.0
    if Phi is None:
        return u
    K = s.shape[1]
    for b in range(K):
        if b == k:
            continue
        lo, hi = min(b, k), max(b, k)
        phi = float(Phi[c, lo * K - lo * (lo + 1) // 2 + (hi - lo - 1)])
        u = u * (1.0 + phi * (1.0 if int(s[c, b, i]) == l else 0.0))
    return u


def split(ell):
    """ell -> (e, mant)."""
    t = (-ell) * LOG2E
    e = math.floor(t)
    return int(e), cexp2(t - e)


def normalise(lp_row, Pi_row, u_row, o, cn_row, coupled):
    """Steps 3-6 for one (chain, dataset, row): dict with ell, p_own, p_new, e, mant, w (list), F; p_own = -1: degenerate."""
    N = len(lp_row)
    lp_row = [float(v) for v in lp_row]
    mx = max(lp_row)
    w = [(cexp(lp_row[l] - mx) * float(Pi_row[l])) * u_row[l] for l in range(N)]
    F = w[0]
    Z0 = float(Pi_row[0]) * u_row[0]
    for l in range(1, N):
        F = F + w[l]
        Z0 = Z0 + float(Pi_row[l]) * u_row[l]
    if not (F > 0.0 and F <= 1.7976931348623157e308):
        return {"ell": float("nan"), "p_own": -1, "p_new": 0, "e": 0, "mant": 0.0, "w": w, "F": F}
    ell = clog(F) + mx
    if coupled:
        ell = ell - clog(Z0)
    q = [int(math.floor(v / F * 1048576.0 + 0.5)) for v in w]
    valid = 0 <= o < N
    p_own = q[o] if valid else 0
    p_new = sum(q[l] for l in range(N) if cn_row[l] == 0 or (valid and l == o and cn_row[l] == 1))
    e, mant = split(ell)
    return {"ell": ell, "p_own": p_own, "p_new": p_new, "e": e, "mant": mant, "w": w, "F": F}


def normalise_all(lp, Pi, s, cnv, Phi):
    """Steps 3-6 everywhere: dict of (C, K, n) arrays ell, p_own, p_new, e, mant."""
    C_, K, n, N = lp.shape
    out = {"ell": np.zeros((C_, K, n)), "p_own": np.zeros((C_, K, n), dtype=np.int64), "p_new": np.zeros((C_, K, n), dtype=np.int64),
           "e": np.zeros((C_, K, n), dtype=np.int64), "mant": np.zeros((C_, K, n))}
    coupled = Phi is not None and K > 1
    for c in range(C_):
        for k in range(K):
            for i in range(n):
                u = [weight_u(s, Phi if coupled else None, c, k, i, l) for l in range(N)]
                r = normalise(lp[c, k, i], Pi[c, k], u, int(s[c, k, i]), cnv[c, k], coupled)
                for name in out:
                    out[name][c, k, i] = r[name]
    return out


BINS = 3


def bin_add(E, S, b, v):
    """The integer v into absolute bin b of the pair (E, S): S the BINS exact sums of bins E, E - 1, E - 2 (Python ints).  A bin
    above E moves the window up, a bin below it is dropped."""
    S = list(S)
    if E == E_EMPTY:
        E, S = b, [0] * BINS
    while b > E:
        E, S = E + 1, [0] + S[:-1]
    if E - b < BINS:
        S[E - b] += v
    return E, S


def pair_add(E, S, e, mant):
    """The term mant 2^e: the integer trunc(mant 2^52) shifted by e mod 32 into bin floor(e / 32)."""
    m = int(mant * 2.0 ** 52) if 0.0 <= mant < 4.0 else 0
    return bin_add(E, S, e // 32, m * 2 ** (e % 32))


def pair_of(ells, batch=None):
    """The pair of a sequence of ell values in order.  batch: sizes of the chain batches the sequence goes through -- they change
    nothing, which is the point."""
    E, S = E_EMPTY, [0] * BINS
    at = 0
    for size in (batch or [len(ells)]):
        for v in ells[at:at + size]:
            E, S = pair_add(E, S, *split(float(v)))
        at += size
    assert at == len(ells)
    return E, S


def pair_merge(a, b):
    """b's pair into a's, bin by bin."""
    E, S = a[0], list(a[1])
    if b[0] != E_EMPTY:
        for j in range(BINS):
            E, S = bin_add(E, S, b[0] - j, b[1][j])
    return E, S


def pack(S):
    """BINS Python ints as the device's 2 BINS int64 words: (high, low) of each 128-bit sum."""
    mask = (1 << 64) - 1
    return np.array([w for v in S for w in ((v >> 64) & mask, v & mask)], dtype=np.uint64).view(np.int64)


def pair_value_log(E, S):
    """log of the pair's sum, from exact integers."""
    total = sum(v << (32 * (BINS - 1 - j)) for j, v in enumerate(S))
    return (32 * (E - (BINS - 1)) - 52) * math.log(2.0) + math.log(total)


class Mirror:
    """Step 7: the sums of everything added so far, from per-row values (the device's own, in the GPU tests)."""
    NAMES = ("own_sum", "new_sum", "zero", "lcp_sum", "lcp_sq_sum", "E", "S")

    def __init__(self, K, n):
        self.K, self.n, self.T = K, n, 0
        self.own_sum, self.new_sum, self.zero = (np.zeros((K, n), dtype=np.int64) for _ in range(3))
        self.lcp_sum, self.lcp_sq_sum = (np.zeros((K, n)) for _ in range(2))
        self.E = np.full((K, n), E_EMPTY, dtype=np.int64)
        self.bins = [[[0] * BINS for _ in range(n)] for _ in range(K)]

    @property
    def S(self):
        return np.array([[pack(self.bins[k][i]) for i in range(self.n)] for k in range(self.K)], dtype=np.int64).reshape(self.K, self.n, 2 * BINS)

    def add(self, ell, p_own, p_new, e=None, mant=None):
        """(C, K, n) each; p_own = -1 marks a degenerate row.  e, mant: the split of ell (the device's own exp2 in the GPU tests);
        None: derived here by the stated rule."""
        C_ = ell.shape[0]
        for k in range(self.K):
            for i in range(self.n):
                lcp, lsq = float(self.lcp_sum[k, i]), float(self.lcp_sq_sum[k, i])
                E, S = int(self.E[k, i]), self.bins[k][i]
                for c in range(C_):
                    if p_own[c, k, i] < 0:
                        self.zero[k, i] += 1
                        continue
                    v = float(ell[c, k, i])
                    self.own_sum[k, i] += int(p_own[c, k, i])
                    self.new_sum[k, i] += int(p_new[c, k, i])
                    lcp = lcp + v
                    lsq = lsq + v * v
                    E, S = pair_add(E, S, *(split(v) if e is None else (int(e[c, k, i]), float(mant[c, k, i]))))
                self.lcp_sum[k, i], self.lcp_sq_sum[k, i], self.E[k, i], self.bins[k][i] = lcp, lsq, E, S
        self.T += 1

    def merge(self, other):
        self.own_sum += other.own_sum
        self.new_sum += other.new_sum
        self.zero += other.zero
        self.lcp_sum = self.lcp_sum + other.lcp_sum
        self.lcp_sq_sum = self.lcp_sq_sum + other.lcp_sq_sum
        for k in range(self.K):
            for i in range(self.n):
                self.E[k, i], self.bins[k][i] = pair_merge((int(self.E[k, i]), self.bins[k][i]), (int(other.E[k, i]), other.bins[k][i]))
        self.T += other.T

    def reset(self):
        self.__init__(self.K, self.n)

    def arrays(self):
        return {name: getattr(self, name) for name in self.NAMES}
