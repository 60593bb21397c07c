"""Closed-form laws of the hyper-parameter updates, written from the reference as it stands (src/update_hypers.jl, align_labels! of
src/misc.jl:61-96, the initialisation and the update order of src/pmdi.jl:59-96,172-185), quirks included:

  * norm_temp is rebuilt from the INITIAL gamma (Gamma_c is made once, src/pmdi.jl:75-79) by update_gamma!, update_Phi! and update_Z;
  * update_gamma! rescales the rows of its norm_temp by gamma'/gamma as it goes, so dataset k sees the datasets before it rescaled;
  * weights -= r log(1 / beta*) in update_Phi!: the mixture weight of shape 1 + r GROWS with beta*;
  * + eps(Float64) on gamma, not on Phi;
  * update_Phi! runs before update_v, so it uses the previous iteration's v.

Every draw is turned into a probability-integral transform u = F(draw | everything that chain drew before it); a correct sampler
gives independent uniform u.  The N^K sums are brute-force numpy sums, the CDFs scipy.special.gammainc; double precision is enough
because the transforms are only binned.  Nothing here imports the oracle, tests/_np_hypers.py, the package or any of their samplers
or random streams: the tests compare those with this file.
"""
from collections import defaultdict

import numpy as np
from scipy import integrate, special, stats

EPS = 2.0 ** -52                      # eps(Float64)
# a gamma draw g is stored as g + EPS: below 2^-90 what g + EPS - EPS gives back is no longer g to the accuracy a bin edge needs
RECOVERABLE = 2.0 ** -90

# the deliberately wrong laws of the sensitivity test (tests/test_exact_hypers.py)
WRONG_LAWS = ("no_boost", "unrescaled_table", "flipped_sign", "stale_Z", "M_prior_scale_4")


def pairs(K):
    return [(a, b) for a in range(K - 1) for b in range(a + 1, K)]


class State:
    """The state one hyper-parameter step starts from.  s: (n, K) labels 1..N; gamma, gamma0: (N, K); Phi: (max(1, K(K-1)/2),)."""

    def __init__(self, s, gamma, gamma0, M, Phi, v, order=None):
        self.s = np.asarray(s, dtype=np.int64)
        self.n, self.K = self.s.shape
        self.gamma, self.gamma0 = np.asarray(gamma, dtype=np.float64), np.asarray(gamma0, dtype=np.float64)
        self.N = self.gamma.shape[0]
        self.M, self.v = np.asarray(M, dtype=np.float64), float(v)
        self.Phi = np.asarray(Phi, dtype=np.float64) if self.K > 1 else np.zeros(1)
        self.order = np.arange(1, self.n + 1) if order is None else np.asarray(order, dtype=np.int64)
        assert self.gamma.shape == self.gamma0.shape == (self.N, self.K) and len(self.M) == self.K
        assert len(self.Phi) == max(1, self.K * (self.K - 1) // 2) and sorted(self.order) == list(range(1, self.n + 1))


def table(g, Phi):
    """exp(norm_temp) of C chains at once: g (C, N, K), Phi (C, npairs) -> (C, N, ..., N), axis 1 + k the label of dataset k:
    prod_k g[c_k, k] * prod over pairs with c_a == c_b of (1 + Phi_ab)."""
    C, N, K = g.shape
    t = np.ones((C,) + (N,) * K)
    for k in range(K):
        shape = [C] + [1] * K
        shape[1 + k] = N
        t = t * g[:, :, k].reshape(shape)
    lab = np.indices((N,) * K)
    for i, (a, b) in enumerate(pairs(K)):
        t = t * (1.0 + Phi[:, i].reshape((C,) + (1,) * K) * (lab[a] == lab[b]))
    return t


def _sum_but(t, keep):
    return t.sum(axis=tuple(ax for ax in range(1, t.ndim) if ax != keep))


def step_transforms(st, out, wrong=None):
    """One step of src/pmdi.jl:176-185 from `st` in C chains.  out: M (C, K), gamma (C, N, K), Phi (C, npairs), v (C,) after the
    step.  Returns (U, floors, Z): U maps a site's name to its (C,) transforms, in the order the reference draws them; floors maps
    a gamma site to the transform below which + eps hides where the draw fell (uniform_counts); Z (C,) is the normalising constant
    update_Z must have found.
    `wrong`: one of WRONG_LAWS, for the sensitivity test."""
    assert wrong is None or wrong in WRONG_LAWS
    N, K, n = st.N, st.K, st.n
    C = out["M"].shape[0]
    counts = np.array([[(st.s[:, k] == m + 1).sum() for k in range(K)] for m in range(N)])
    g0 = np.broadcast_to(st.gamma0, (C, N, K))
    Phi0 = np.broadcast_to(st.Phi, (C, len(st.Phi)))
    U, floors = {}, {}
    # update_gamma! (update_hypers.jl:64-92): Gamma(M'_k / N + count, scale 1 / beta*) + eps, beta* = 1 + v S / gamma[m, k]
    scaled = np.array(g0)
    for k in range(K):
        t = table(g0 if wrong == "unrescaled_table" else scaled, Phi0)
        beta = 1.0 + st.v * _sum_but(t, 1 + k) / st.gamma[:, k]
        shape = out["M"][:, k:k + 1] / N + counts[:, k]
        law_shape = np.where(shape < 1.0, shape + 1.0, shape) if wrong == "no_boost" else shape
        for m in range(N):
            x = np.maximum(out["gamma"][:, m, k] - EPS, 0.0) * beta[:, m]
            U[f"gamma[{m},{k}]"] = special.gammainc(law_shape[:, m], x)
            floors[f"gamma[{m},{k}]"] = float(special.gammainc(shape[:, m], RECOVERABLE * beta[:, m]).max())
        scaled[:, :, k] = g0[:, :, k] * out["gamma"][:, :, k] / st.gamma[:, k]
    # update_Phi! (:95-128): alpha* = 1 + r, r ~ w_r; Gamma(alpha*, scale 1 / beta*), beta* = 5 + v S_ab / (1 + Phi_ab)
    Phi_cur = np.array(Phi0)
    lab = np.indices((N,) * K)
    for i, (a, b) in enumerate(pairs(K)):
        t = table(g0, Phi_cur)
        S = (t * (lab[a] == lab[b])).reshape(C, -1).sum(axis=1)
        beta = 5.0 + st.v * S / (1.0 + st.Phi[i])
        n_agree = int((st.s[:, a] == st.s[:, b]).sum())
        r = np.arange(n_agree + 1)
        sign = -1.0 if wrong == "flipped_sign" else 1.0
        logw = special.gammaln(r + 1.0) + stats.binom.logpmf(r, n_agree, 0.5) + sign * r * np.log(beta)[:, None]
        w = np.exp(logw - logw.max(axis=1, keepdims=True))
        w /= w.sum(axis=1, keepdims=True)
        U[f"Phi[{i}]"] = (w * special.gammainc(1.0 + r, (out["Phi"][:, i] * beta)[:, None])).sum(axis=1)
        Phi_cur[:, i] = out["Phi"][:, i]
    # update_Z (:29-39) with the initial gamma and the new Phi; update_v (:1-3): Gamma(n, scale 1 / Z')
    Z = table(g0, out["Phi"]).reshape(C, -1).sum(axis=1)
    Z_law = table(g0, Phi0).reshape(C, -1).sum(axis=1) if wrong == "stale_Z" else Z
    U["v"] = special.gammainc(float(n), out["v"] * Z_law)
    return U, floors, Z


class MLaw:
    """update_M! (update_hypers.jl:5-26) for one dataset: propose x ~ Normal(M, 0.1^2), accept with min(1, pi(x) / pi(M)) for x > 0,
    log pi(m) = sum_l logpdf(Gamma(m / N, 1), gamma[l]) + logpdf(Gamma(2, scale 0.25), m).  density(x) is the sub-density of a MOVE
    to x; it integrates to the probability of moving at all."""
    HALF_WIDTH = 1.2                  # 12 standard deviations of the proposal: what lies outside is below 1e-32

    def __init__(self, M, gamma_col, prior_scale=0.25):
        self.M, self.g, self.N, self.scale = float(M), np.asarray(gamma_col, dtype=np.float64), len(gamma_col), prior_scale
        self.lo, self.hi = max(0.0, self.M - self.HALF_WIDTH), self.M + self.HALF_WIDTH
        self.p_move = self.mass(self.lo, self.hi)

    def logpi(self, m):
        a = m / self.N
        return float((-special.gammaln(a) + (a - 1.0) * np.log(self.g) - self.g).sum() + np.log(m) - m / self.scale)

    def density(self, x):
        if x <= 0.0:
            return 0.0
        return min(1.0, np.exp(self.logpi(x) - self.logpi(self.M))) * stats.norm.pdf(x, self.M, 0.1)

    def mass(self, lo, hi):
        lo, hi = max(lo, self.lo), min(hi, self.hi)
        if hi <= lo:
            return 0.0
        pts = [p for p in (self.M,) if lo < p < hi]
        return integrate.quad(self.density, lo, hi, points=pts or None, limit=200, epsabs=1e-13, epsrel=1e-11)[0]

    def edges(self):
        """Fixed bins of the moved values: half proposal standard deviations out to +-2.5, and the two tails."""
        return np.concatenate([[self.lo], self.M + 0.05 * np.arange(-5, 6), [self.hi]])

    def moved_counts(self, values):
        """Moved values -> (observed, expected) counts on edges(), expected = share of the move sub-density."""
        e = self.edges()
        e = e[(e >= self.lo) & (e <= self.hi)]
        e = np.unique(e)
        obs = np.histogram(values, bins=e)[0]
        assert obs.sum() == len(values), "a moved M outside the proposal's reach"
        prob = np.array([self.mass(a, b) for a, b in zip(e[:-1], e[1:])])
        return obs, prob / prob.sum() * len(values)


def binomial_pvalue(k, n, p):
    return float(stats.binomtest(int(k), int(n), float(p)).pvalue)


def uniform_counts(u, bins, floor=0.0):
    """Counts of u on `bins` equal-width bins of [0, 1] against the uniform law.  Bins that end at or below `floor` are joined to the
    bin that `floor` lies in: below `floor` a stored draw no longer says where in the bin it fell, only that it fell there."""
    u = np.asarray(u, dtype=np.float64)
    assert np.isfinite(u).all() and (u >= 0).all() and (u <= 1).all()
    idx = np.minimum((u * bins).astype(np.int64), bins - 1)
    obs = np.bincount(idx, minlength=bins).astype(np.float64)
    exp = np.full(bins, len(u) / bins)
    first = min(int(floor * bins), bins - 1)              # the bin `floor` lies in
    if first > 0:
        obs = np.concatenate([[obs[:first + 1].sum()], obs[first + 1:]])
        exp = np.concatenate([[exp[:first + 1].sum()], exp[first + 1:]])
    return obs, exp


def pair_counts(u1, u2, side=4):
    """side x side contingency table of two transforms against the product of their (uniform) laws."""
    a = np.minimum((np.asarray(u1) * side).astype(np.int64), side - 1)
    b = np.minimum((np.asarray(u2) * side).astype(np.int64), side - 1)
    return np.bincount(a * side + b, minlength=side * side), np.full(side * side, len(a) / side ** 2)


def shuffle_tables(order, group=1):
    """order: (C, n) 1-based outputs of shuffle!.  A uniform permutation puts every element at every position with probability 1 / n
    and every ordered pair of distinct elements at positions (0, 1) with probability 1 / (n (n - 1)).  -> [(name, obs, exp)].
    The first table holds n counts per chain whose row and column sums are fixed, so its Pearson statistic is stochastically SMALLER
    than the chi-square law it is compared with (mean n (n - 1), not n^2 - 1): a correct shuffle fails it less often than p says.
    group > 1 pools elements into blocks of `group` consecutive values in the pair tables (n (n - 1) cells would be empty)."""
    order = np.asarray(order) - 1
    C, n = order.shape
    assert (np.sort(order, axis=1) == np.arange(n)).all(), "not a permutation"
    out = [("element x position", np.bincount((order * n + np.arange(n)).ravel(), minlength=n * n), np.full(n * n, C / n))]
    G = -(-n // group)
    size = np.bincount(np.arange(n) // group, minlength=G).astype(np.float64)
    expect = (np.outer(size, size) - np.diag(size)) / (n * (n - 1.0)) * C
    spots = [(0, 1)] + ([(n - 1, n - 257)] if n > 256 else [])       # the second: either side of the first 256-position chunk
    for p, q in spots:
        obs = np.bincount((order[:, p] // group) * G + order[:, q] // group, minlength=G * G)
        keep = expect.ravel() > 0
        out.append((f"pair at positions {p},{q}", obs[keep], expect.ravel()[keep]))
        assert obs[~keep].sum() == 0
    return out


def init_transforms(n, out):
    """src/pmdi.jl:59-66,95-96.  out: gamma0 (C, N, K) as drawn, Phi (C, npairs), s (C, n, K), v (C,).  -> (U, floors, Z, s_tables):
    gamma0 ~ Gamma(1 / N, 1) + eps, Phi ~ Gamma(1, scale 0.2), v ~ Gamma(n, scale 1 / Z); s_tables[k] = (observed, expected) label
    counts of dataset k over all chains, expected from each chain's own gamma0[:, k] / sum."""
    C, N, K = out["gamma0"].shape
    U, floors = {}, {}
    for k in range(K):
        for m in range(N):
            U[f"gamma0[{m},{k}]"] = special.gammainc(1.0 / N, np.maximum(out["gamma0"][:, m, k] - EPS, 0.0))
            floors[f"gamma0[{m},{k}]"] = float(special.gammainc(1.0 / N, RECOVERABLE))
    for i in range(len(pairs(K))):
        U[f"Phi[{i}]"] = special.gammainc(1.0, out["Phi"][:, i] / 0.2)
    Phi = out["Phi"] if K > 1 else np.zeros((C, 1))
    Z = table(out["gamma0"], Phi).reshape(C, -1).sum(axis=1)
    U["v"] = special.gammainc(float(n), out["v"] * Z)
    s_tables = []
    for k in range(K):
        p = out["gamma0"][:, :, k] / out["gamma0"][:, :, k].sum(axis=1, keepdims=True)
        obs = np.bincount((out["s"][:, :, k] - 1).ravel(), minlength=N)
        s_tables.append((obs, n * p.sum(axis=0)))
    return U, floors, Z, s_tables


def align_law(s, Phi, N):
    """The exact law of align_labels! (src/misc.jl:61-96) on allocations s (n, K): for k, for label in unique(s[:, k]) (order of
    first appearance, taken once per k), for new_label in 1:N; every proposal is accepted with probability
    min(1, exp(swap - keep)) and the accepted label is carried on.  The outcome is K permutations sigma_k of the labels
    (s[:, k] <- sigma_k[s[:, k]], gamma[sigma_k[m], k] <- gamma[m, k]).
    -> ({(sigma_0, ..., sigma_K-1): probability}, [(acceptance probability, probability of reaching that proposal)])."""
    s0 = np.asarray(s, dtype=np.int64) - 1
    n, K = s0.shape
    logphi = np.log1p(np.asarray(Phi, dtype=np.float64))
    pair_of = {p: i for i, p in enumerate(pairs(K))}
    ident = tuple(range(N))
    dist, reached = {(ident,) * K: 1.0}, []
    if K == 1:
        return dist, reached
    for k in range(K):
        occupied = list(dict.fromkeys(int(x) for x in s0[:, k]))          # sigma_k is still the identity here
        for first in occupied:
            cur = {}
            for sig, p in dist.items():
                live = bool((np.asarray(sig[k])[s0[:, k]] == first).any())  # all(label_ind .== false) && continue
                cur[(sig, first if live else -1)] = p
            for new in range(N):
                nxt = defaultdict(float)
                for (sig, label), p in cur.items():
                    if label < 0 or new == label:
                        nxt[(sig, label)] += p
                        continue
                    sk = np.asarray(sig[k])[s0[:, k]]
                    lm, nm = sk == label, sk == new
                    keep = swap = 0.0
                    for j in range(K):
                        if j == k:
                            continue
                        sj = np.asarray(sig[j])[s0[:, j]]
                        w = logphi[pair_of[(min(j, k), max(j, k))]]
                        keep += w * ((sj[lm] == label).sum() + (sj[nm] == new).sum())
                        swap += w * ((sj[lm] == new).sum() + (sj[nm] == label).sum())
                    acc = min(1.0, float(np.exp(swap - keep)))
                    reached.append((acc, p))
                    swapped = tuple(new if x == label else label if x == new else x for x in sig[k])
                    nxt[(sig[:k] + (swapped,) + sig[k + 1:], new)] += p * acc
                    nxt[(sig, label)] += p * (1.0 - acc)
                cur = {key: p for key, p in nxt.items() if p > 0.0}
            dist = defaultdict(float)
            for (sig, _), p in cur.items():
                dist[sig] += p
            dist = dict(dist)
    assert abs(sum(dist.values()) - 1.0) < 1e-12
    return dist, reached


def align_outcomes(s_in, gamma_in, s_out, gamma_out):
    """C chains' aligned states -> list of their (sigma_0, ..., sigma_K-1), read off where each (distinct) gamma value went; the
    allocations must have moved with them."""
    s_in, gamma_in = np.asarray(s_in), np.asarray(gamma_in)
    N, K = gamma_in.shape
    assert all(len(set(gamma_in[:, k])) == N for k in range(K)), "the gamma values of a dataset must be distinct"
    res = []
    for c in range(len(s_out)):
        sig = []
        for k in range(K):
            where = [np.nonzero(gamma_out[c][:, k] == gamma_in[m, k])[0] for m in range(N)]
            assert all(len(w) == 1 for w in where), "gamma is not a permutation of its rows"
            sk = np.array([int(w[0]) for w in where])
            assert (s_out[c][:, k] - 1 == sk[s_in[:, k] - 1]).all(), "allocations and gamma rows were not exchanged together"
            sig.append(tuple(int(x) for x in sk))
        res.append(tuple(sig))
    return res
