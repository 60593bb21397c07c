"""Closed-form laws of one swept observation, in 50-digit arithmetic (mpmath), restated from the reference's cluster definitions
(src/datatypes/{gaussian,categorical,negbinom}_cluster.jl) as the distributions they ARE -- not as the recursions the code runs:

  Gaussian     Normal-inverse-gamma prior (mu_0 = 0, kappa_0 = 0.001, alpha_0 = beta_0 = 0.5) per feature; the predictive of a cluster
               holding m members is Student-t with m + 1 degrees of freedom, computed from the members' raw values by a two-pass
               mean / sum of squares.  An EMPTY cluster is the reference's constructor (mu = 0, lambda = 1: a standard Cauchy), which
               is not the m -> 0 limit of the formula -- the reference defines it so.
  Categorical  (count + 1/2) / (m + L_q / 2), L_q the largest level of feature q in the whole dataset.
  NegBinom     (m + 1) B(x + S + 1, m + 2) / B(S + 1, m + 1) as an exact product of integers (no gamma function at all).

and the law of the step of src/pmdi.jl:209-314 when every particle holds the same clusters: labels drawn from
f_k(c) = Pi[c, k] pred_k,c(x) / sum_c', log-weight lw_init + sum_k log sum_c Pi[c, k] pred_k,c(x) + sum over dataset pairs with equal
labels of log(1 + Phi_kl).

Nothing here imports the oracle, the package or any restated sweep: the tests compare those with this file.
"""
import numpy as np
from mpmath import mp, mpf

mp.dps = 50

KAPPA0, ALPHA0, BETA0 = mpf("0.001"), mpf("0.5"), mpf("0.5")


def logsumexp(v):
    m = max(v)
    return m + mp.log(sum(mp.exp(x - m) for x in v))


def gaussian_logpred(members, x, flag=None):
    """members: (m, D) raw rows of the cluster, x: (D,) the new row; features with flag 0 do not exist."""
    members = np.asarray(members, dtype=np.float64).reshape(-1, len(x))
    m = members.shape[0]
    nu = mpf(m + 1)
    out = mpf(0)
    for q in range(len(x)):
        if flag is not None and not flag[q]:
            continue
        if m == 0:
            mu, lam = mpf(0), mpf(1)
        else:
            col = [mpf(float(v)) for v in members[:, q]]
            mean = sum(col) / m
            ss = sum((v - mean) ** 2 for v in col)
            kappa = KAPPA0 + m
            mu = m * mean / kappa
            beta = BETA0 + ss / 2 + KAPPA0 * m * mean ** 2 / (2 * kappa)
            lam = (ALPHA0 + mpf(m) / 2) * kappa / (beta * (kappa + 1))
        d = mpf(float(x[q])) - mu
        out += (mp.loggamma((nu + 1) / 2) - mp.loggamma(nu / 2) - mp.log(mp.pi * nu) / 2 + mp.log(lam) / 2
                - (nu + 1) / 2 * mp.log(1 + lam * d * d / nu))
    return out


def categorical_logpred(members, x, levels, flag=None):
    """levels: (D,) largest level of each feature over the whole dataset."""
    members = np.asarray(members, dtype=np.int64).reshape(-1, len(x))
    m = members.shape[0]
    out = mpf(0)
    for q in range(len(x)):
        if flag is not None and not flag[q]:
            continue
        cnt = int((members[:, q] == int(x[q])).sum())
        out += mp.log((mpf(cnt) + mpf("0.5")) / (mpf(m) + mpf(int(levels[q])) / 2))
    return out


def negbinom_logpred(members, x, flag=None):
    members = np.asarray(members, dtype=np.int64).reshape(-1, len(x))
    m = members.shape[0]
    out = mpf(0)
    for q in range(len(x)):
        if flag is not None and not flag[q]:
            continue
        S, xo = int(members[:, q].sum()), int(x[q])
        num = mpf(m + 1)
        for j in range(1, xo + 1):
            num *= S + j
        den = mpf(1)
        for j in range(xo + 1):
            den *= S + m + 2 + j
        out += mp.log(num / den)
    return out


def logpred(kind, data, member_rows, row, flag=None):
    members = data[list(member_rows)]
    if kind == "gaussian":
        return gaussian_logpred(members, data[row], flag)
    if kind == "categorical":
        return categorical_logpred(members, data[row], data.max(axis=0), flag)
    if kind == "negbinom":
        return negbinom_logpred(members, data[row], flag)
    raise ValueError(kind)


def phi_pairs(K):
    return [(a, b) for a in range(K - 1) for b in range(a + 1, K)]


class StepLaw:
    """The law of sweeping observation `row` when the observations `prefix_rows` sit in the clusters `prefix_labels` (m, K), 1-based.
    f[k][c]: probability that a free particle draws label c + 1 in dataset k; logZ[k]: the log-weight increment of dataset k."""

    def __init__(self, data, kinds, N, prefix_rows, prefix_labels, row, Pi, Phi, flags=None):
        K = len(data)
        prefix_rows = np.asarray(prefix_rows, dtype=np.int64)
        prefix_labels = np.asarray(prefix_labels, dtype=np.int64).reshape(len(prefix_rows), K)
        self.K, self.N = K, N
        self.Phi = [mpf(float(v)) for v in np.atleast_1d(Phi)]
        self.f, self.logZ, self.prefix_count = [], [], np.zeros((K, N), dtype=np.int64)
        for k in range(K):
            terms = []
            for c in range(1, N + 1):
                rows = prefix_rows[prefix_labels[:, k] == c]
                self.prefix_count[k, c - 1] = len(rows)
                fl = None if flags is None else flags[k]
                terms.append(mp.log(mpf(float(Pi[c - 1, k]))) + logpred(kinds[k], data[k], rows, row, fl))
            z = logsumexp(terms)
            self.logZ.append(z)
            self.f.append([mp.exp(t - z) for t in terms])

    def f_float(self, k):
        return np.array([float(v) for v in self.f[k]])

    def logweight(self, labels, lw_init):
        """labels: (K,) 1-based labels of one particle -> its exact log-weight after the step."""
        out = mpf(lw_init) + sum(self.logZ)
        for i, (a, b) in enumerate(phi_pairs(self.K)):
            if labels[a] == labels[b]:
                out += mp.log(1 + self.Phi[i])
        return out


# ---- cases and statistics shared by tests/test_exact_step.py (oracle) and tests/test_gpu_exact_step.py (HIP kernels) -----------------

KIND_SETS = [("gaussian",), ("categorical",), ("negbinom",), ("gaussian", "categorical"), ("categorical", "negbinom"),
             ("gaussian", "gaussian", "gaussian"), ("gaussian", "categorical", "negbinom")]
N_OBS = {2: 12, 10: 40, 64: 80}         # observations per number of labels (N <= n, src/pmdi.jl:54)
PARTICLES = (256, 1024, 2048, 4096)
P_FLOOR = 1e-6                          # every statistical assertion: p-value >= P_FLOOR


def make_data(rng, kind, n):
    z = rng.integers(0, 3, n)
    if kind == "gaussian":
        return rng.normal(size=(n, 5)) + 1.5 * (z[:, None] - 1)
    if kind == "categorical":
        return (1 + (rng.random((n, 4)) < 0.25 + 0.25 * z[:, None]) + (z[:, None] == 2) * rng.integers(0, 3, (n, 4))).astype(np.int64)
    return (rng.geometric(0.25 + 0.2 * z[:, None], size=(n, 3)) - 1).astype(np.int64)


class StepCase:
    """One swept observation (n1 = n) or two (n1 = n - 1) behind a prefix of known labels.  `variant` picks, deterministically, the
    feature flags (odd: about a third of the features off), the prefix (0: labels spread over at most min(N, 5) of the N labels, the rest
    empty -> prior predictive; 1: one label holds everything; 2: spread over all N) and the first-iteration log-weight (variant 3)."""

    def __init__(self, kinds, N, P, variant, swept=1, phi=None):
        self.kinds, self.N, self.P, self.K = list(kinds), N, P, len(kinds)
        self.n = n = N_OBS[N]
        rng = np.random.default_rng([N, P, variant, swept] + [len(k) for k in kinds])
        self.data = [make_data(rng, kind, n) for kind in kinds]
        self.flags = None
        if variant % 2:
            self.flags = [(rng.random(d.shape[1]) < 0.67).astype(np.uint8) for d in self.data]
            for f in self.flags:
                f[0] = 1
        used = (min(N, 5), 1, N)[variant % 3]
        lab = rng.permutation(N)[:used] + 1
        self.s = lab[rng.integers(0, used, size=(n, self.K))]
        self.order = rng.permutation(n) + 1
        self.n1 = n - swept + 1
        Pi = rng.gamma(2.0, 1.0, size=(N, self.K)) if variant % 2 == 0 else rng.gamma(4.0 / N, 1.0, size=(N, self.K)) + 1e-3
        self.Pi = Pi / Pi.sum(0)
        npairs = max(1, self.K * (self.K - 1) // 2)
        self.Phi = rng.uniform(0.05, 0.5, size=npairs) if phi is None else np.full(npairs, float(phi))
        if self.K == 1:
            self.Phi = np.zeros(1)
        self.it = 1 if variant == 3 else 2 + variant
        self.lw_init = 0.0 if self.it == 1 else 1.0          # src/pmdi.jl:99,372
        self.prefix_rows = self.order[:self.n1 - 1] - 1
        self.row = int(self.order[self.n1 - 1] - 1)           # the (first) swept observation
        self.flags_flat = None if self.flags is None else np.concatenate(self.flags)

    def law(self, Pi=None):
        return StepLaw(self.data, self.kinds, self.N, self.prefix_rows, self.s[self.prefix_rows], self.row,
                       self.Pi if Pi is None else Pi, self.Phi, self.flags)

    def tolerance(self, value, negbinom_ulps):
        """Gaussian: 1e-12 relative; Categorical: 4 units in the last place of the exact value; NegBinom: `negbinom_ulps` of them."""
        tol = 0.0
        if "gaussian" in self.kinds:
            tol += 1e-12 * abs(value)
        if "negbinom" in self.kinds:
            tol += negbinom_ulps * float(np.spacing(abs(value)))
        elif "categorical" in self.kinds:
            tol += 4 * float(np.spacing(abs(value)))
        return tol


def weight_cases():
    """Every cluster-type set x N x P, flags / prefix / first-iteration variants cycling: 84 cases."""
    out, i = [], 0
    for kinds in KIND_SETS:
        for N in (2, 10, 64):
            for P in PARTICLES:
                out.append((kinds, N, P, i % 6))
                i += 1
    return out


def draw_cases():
    """Every cluster-type set x N, P and the variants cycling: 21 cases."""
    out, i = [], 0
    for kinds in KIND_SETS:
        for N in (2, 10, 64):
            out.append((kinds, N, PARTICLES[i % 4], (i // 2) % 6))
            i += 1
    return out


def case_id(c):
    return "+".join(k[:3] for k in c[0]) + f"-N{c[1]}-P{c[2]}-v{c[3]}"


def labels_from_export(state, prefix_count, added=1):
    """(P, K) labels drawn at the swept observation, read off an exported state: in every particle exactly one label's cluster has
    grown by one member over the prefix.  state: particle (K, P, N) 1-based ids, cluster_n (K, cap) indexed id - 1."""
    K, P, N = state["particle"].shape
    lab = np.zeros((P, K), dtype=np.int64)
    for k in range(K):
        grown = state["cluster_n"][k][state["particle"][k] - 1] - prefix_count[k][None, :]
        assert ((grown == 0) | (grown == added)).all() and ((grown == added).sum(axis=1) == 1).all(), \
            f"dataset {k}: a particle's clusters do not hold the prefix plus the swept observation in one label"
        lab[:, k] = np.argmax(grown, axis=1) + 1
    return lab


def chi2_pvalue(observed, expected):
    """Pearson chi-square of counts against expected counts; bins with expected < 10 pooled into one (joined to the smallest
    other bin if the pool itself stays below 10).  Returns (p, number of bins)."""
    from scipy.stats import chi2
    o, e = np.asarray(observed, dtype=np.float64).ravel(), np.asarray(expected, dtype=np.float64).ravel()
    assert abs(o.sum() - e.sum()) < 1e-6 * max(1.0, e.sum())
    big = e >= 10
    ob, eb = list(o[big]), list(e[big])
    if (~big).any():
        op, ep = o[~big].sum(), e[~big].sum()
        if ep >= 10 or not eb:
            ob.append(op); eb.append(ep)
        else:
            j = int(np.argmin(eb))
            ob[j] += op; eb[j] += ep
    ob, eb = np.array(ob), np.array(eb)
    if len(eb) < 2:
        return 1.0, len(eb)
    stat = ((ob - eb) ** 2 / eb).sum()
    return float(chi2.sf(stat, len(eb) - 1)), len(eb)


def systematic_family_contains(weights, keys_before, keys_after):
    """Is `keys_after` an outcome of the reference's resampling (src/misc.jl:27-47) of particles with normalised `weights` and
    per-particle keys `keys_before`?  That family: ancestors a_i = first p with W_p >= u + i/P for SOME u in (0, 1/P) (so every
    ancestor has floor(P w) or ceil(P w) offspring), then one slot dropped and particle 0 put in front.  The unknown u is searched
    over the <= P + 1 intervals on which the ancestor vector is constant."""
    P = len(weights)
    W = np.cumsum(np.asarray(weights, dtype=np.longdouble))
    PW = np.asarray(W / W[-1] * P, dtype=np.float64)
    PW[-1] = P
    frac = np.unique(np.concatenate([[0.0, 1.0], PW - np.floor(PW)]))
    after = np.asarray(keys_after)
    if after[0] != keys_before[0]:
        return False
    for v in (frac[:-1] + frac[1:]) / 2:
        a = np.searchsorted(PW, v + np.arange(P), side="left")
        T = np.asarray(keys_before)[np.minimum(a, P - 1)]
        ne_front = np.nonzero(T[:P - 1] != after[1:])[0]
        pre = ne_front[0] if ne_front.size else P - 1          # T[:pre] == after[1:pre+1]
        ne_back = np.nonzero(T[1:] != after[1:])[0]
        suf = (P - 1) - (ne_back[-1] + 1) if ne_back.size else P - 1
        if pre + suf >= P - 1:
            return True
    return False
