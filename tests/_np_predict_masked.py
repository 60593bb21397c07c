"""The yardstick of the masked add and the imputation sums of the predictive accumulator (include/pmdi_hip.h, "Masked add",
"Imputation sums"): _np_predict's mirror with one change -- the oracle's calc_logprob gets flags .& observed[j] per new row.
Clusters are built by the CPU oracle's cluster_add! in ascending row order under the chain's flags alone (the mask never touches
the training data), mu comes from the oracle's cluster statistics, and the imputation sums are Python float loops in the stated
order (impute_entry); impute_sums does the same operations on whole (row, feature) arrays, one label at a time, which
tests/test_predict_masked_host.py holds to the loops bit for bit.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import _np_predict as X

Q_ONE = X.Q_ONE


def log_predictives(O, train, kinds, new, observed, s, flags, N, want_mu=False):
    """lp (C, K, m, N), empty (C, K, N) and, with want_mu, mu (C, K, N, Dmax) of the Gaussian datasets (0 elsewhere).  observed:
    K boolean (m, D_k) masks or None entries.  Values at unobserved entries are replaced by a valid filler before the oracle sees
    the stacked matrix (it reads whole rows); the narrowed flag keeps them out of the result."""
    C_, K, n = s.shape
    m = new[0].shape[0]
    D = [x.shape[1] for x in train]
    Dmax = max([1] + [d for d, kind in zip(D, kinds) if kind == "gaussian"])
    lp = np.zeros((C_, K, m, N))
    empty = np.zeros((C_, K, N), dtype=bool)
    mu = np.zeros((C_, K, N, Dmax))
    both = []
    for k in range(K):
        y = np.array(new[k])
        if observed[k] is not None:
            y = np.where(observed[k], y, 0.0 if kinds[k] == "gaussian" else (1 if kinds[k] == "categorical" else 0)).astype(train[k].dtype)
        if kinds[k] == "categorical":
            assert (y.max(axis=0) <= train[k].max(axis=0)).all(), "a new level above the training column's maximum"
        both.append(np.concatenate([train[k], y], axis=0))
    for c in range(C_):
        fl = X.split_flags(None if flags is None else flags[c], D)
        for k in range(K):
            base = np.ones(D[k], dtype=np.uint8) if fl[k] is None else fl[k]
            rowflags = None if observed[k] is None else [np.ascontiguousarray(base & observed[k][j].astype(np.uint8)) for j in range(m)]
            for l in range(N):
                members = np.flatnonzero(s[c, k] == l)          # ascending
                empty[c, k, l] = members.size == 0
                cl = O.Cluster(both[k], kinds[k])
                for i in members:
                    cl.add(int(i), fl[k])
                lp[c, k, :, l] = [cl.logprob(n + j, fl[k] if rowflags is None else rowflags[j]) for j in range(m)]
                if want_mu and kinds[k] == "gaussian":
                    mu[c, k, l, :D[k]] = cl.stats()["mu"]
    return (lp, empty, mu) if want_mu else (lp, empty)


def impute_entry(q_col, mu_col):
    """e of one (chain, new row, feature): q_col the N weights of the row, mu_col the N locations of the feature."""
    e = 0.0
    for qv, mv in zip(q_col, mu_col):
        e = e + float(int(qv)) * float(mv)
    return e


def impute_sums_loops(loc, flag_on, q, mu, flags, kinds, D, count=True):
    """One add into loc (m, sumD) and flag_on (sumD,) in place, entry by entry with Python floats: chains ascending, only where the
    chain has the feature on.  q (C, K, m, N) integers, mu (C, K, N, Dmax), flags (C, sumD) or None."""
    C_, K, m, N = q.shape
    at = np.concatenate([[0], np.cumsum(D)])
    for k in range(K):
        if kinds[k] != "gaussian":
            continue
        for f in range(D[k]):
            col = int(at[k]) + f
            for c in range(C_):
                if flags is not None and not flags[c, col]:
                    continue
                if count:
                    flag_on[col] += 1
                for j in range(m):
                    loc[j, col] = float(loc[j, col]) + impute_entry(q[c, k, j], mu[c, k, :, f])


def impute_sums(loc, flag_on, q, mu, flags, kinds, D, count=True):
    """impute_sums_loops with the (row, feature) entries of a dataset carried as arrays: per label one product and one sum of
    float64 arrays (two roundings per entry and label, as the loops), labels and chains in the same order."""
    C_, K, m, N = q.shape
    at = np.concatenate([[0], np.cumsum(D)])
    for k in range(K):
        if kinds[k] != "gaussian":
            continue
        cols = slice(int(at[k]), int(at[k + 1]))
        for c in range(C_):
            e = np.zeros((m, D[k]))
            qd = q[c, k].astype(np.float64)
            for l in range(N):
                prod = qd[:, l, None] * mu[c, k, l, None, :D[k]]
                e = e + prod
            on = np.ones(D[k], dtype=bool) if flags is None else flags[c, cols].astype(bool)
            loc[:, cols] = np.where(on[None, :], loc[:, cols] + e, loc[:, cols])
            if count:
                flag_on[cols] += on
    return loc, flag_on


def null_locations(train, kinds):
    """(sumD,): Sigma / (n + 0.001) of the cluster that holds every observation, rows added in ascending order; 0 for the other kinds."""
    out = []
    for x, kind in zip(train, kinds):
        v = np.zeros(x.shape[1])
        if kind == "gaussian":
            for q in range(x.shape[1]):
                acc = 0.0
                for i in range(x.shape[0]):
                    acc = acc + float(x[i, q])
                v[q] = acc / (x.shape[0] + 0.001)
        out.append(v)
    return np.concatenate(out)


def fitted(loc, flag_on, null_loc, TC):
    return (loc / float(Q_ONE) + ((TC - flag_on) * null_loc)[None, :]) / TC


class ImputeMirror:
    """The imputation sums of everything added so far."""

    def __init__(self, m, kinds, D, coupled=False):
        self.m, self.kinds, self.D, self.coupled = m, list(kinds), list(D), coupled
        self.loc_sum = np.zeros((m, sum(D)))
        self.loc_joint_sum = np.zeros((m, sum(D))) if coupled else None
        self.flag_on = np.zeros(sum(D), dtype=np.int64)

    def add(self, q, mu, flags, qj=None):
        impute_sums(self.loc_sum, self.flag_on, q, mu, flags, self.kinds, self.D)
        if self.coupled:
            impute_sums(self.loc_joint_sum, self.flag_on, qj, mu, flags, self.kinds, self.D, count=False)

    def merge(self, other):
        self.loc_sum = self.loc_sum + other.loc_sum
        if self.coupled:
            self.loc_joint_sum = self.loc_joint_sum + other.loc_joint_sum
        self.flag_on += other.flag_on

    def reset(self):
        self.__init__(self.m, self.kinds, self.D, self.coupled)

    def arrays(self):
        out = {"loc_sum": self.loc_sum, "flag_on": self.flag_on}
        if self.coupled:
            out["loc_joint_sum"] = self.loc_joint_sum
        return out
