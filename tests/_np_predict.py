"""The yardstick of the predictive accumulator (include/pmdi_hip.h, pmdi_predict_*): a plain numpy / Python mirror of the four
steps of one add.  Clusters are built by the CPU oracle's cluster_add! in ascending row order under the chain's flags and
evaluated by its calc_logprob; the proposal weights are Python float loops, the sums Python integers and a float loop in chain
order.  TEST INFRASTRUCTURE ONLY."""
import math

import numpy as np

Q_ONE = 1 << 20


def split_flags(flags_row, D):
    """One chain's (sumD,) flag bytes as a list of per-dataset arrays; None stays None (every feature on)."""
    if flags_row is None:
        return [None] * len(D)
    at = np.concatenate([[0], np.cumsum(D)])
    return [np.ascontiguousarray(flags_row[at[k]:at[k + 1]], dtype=np.uint8) for k in range(len(D))]


def log_predictives(O, train, kinds, new, s, flags, N):
    """Steps 1 and 2: lp (C, K, m, N) float64 and empty (C, K, N) bool.  train / new: lists of K matrices (n, D_k) / (m, D_k);
    s (C, K, n) 0-based labels; flags (C, sumD) bytes or None.  The oracle's cluster reads rows of ONE matrix, so the new rows
    are stacked under the training rows; that must not change a categorical column's maximum (its nlevels)."""
    C_, K, n = s.shape
    m = new[0].shape[0]
    D = [x.shape[1] for x in train]
    lp = np.zeros((C_, K, m, N))
    empty = np.zeros((C_, K, N), dtype=bool)
    both = []
    for k in range(K):
        if kinds[k] == "categorical":
            assert (new[k].max(axis=0) <= train[k].max(axis=0)).all(), "a new level above the training column's maximum"
        both.append(np.concatenate([train[k], new[k]], axis=0))
    prior = {}                                   # the constructor's cluster under a flag pattern: the same for every empty label
    for c in range(C_):
        fl = split_flags(None if flags is None else flags[c], D)
        for k in range(K):
            key = (k, None if fl[k] is None else fl[k].tobytes())
            for l in range(N):
                members = np.flatnonzero(s[c, k] == l)          # ascending
                empty[c, k, l] = members.size == 0
                if members.size == 0 and key in prior:
                    lp[c, k, :, l] = prior[key]
                    continue
                cl = O.Cluster(both[k], kinds[k])
                for i in members:
                    cl.add(int(i), fl[k])
                col = np.array([cl.logprob(n + j, fl[k]) for j in range(m)])
                lp[c, k, :, l] = col
                if members.size == 0:
                    prior[key] = col
    return lp, empty


def proposal(lp_row, Pi_row):
    """Step 3 for one (chain, dataset, new row): (q list of Python ints, inc float), the stated operations in the stated order."""
    lp_row = [float(v) for v in lp_row]
    mx = max(lp_row)
    f = [math.exp(v - mx) * float(p) for v, p in zip(lp_row, Pi_row)]
    F = f[0]
    for v in f[1:]:
        F = F + v
    inc = math.log(F) + mx
    q = [int(math.floor(v / F * 1048576.0 + 0.5)) for v in f]
    return q, inc


def proposals(lp, Pi):
    """Step 3 everywhere: q (C, K, m, N) int64, inc (C, K, m) float64."""
    C_, K, m, N = lp.shape
    q = np.zeros((C_, K, m, N), dtype=np.int64)
    inc = np.zeros((C_, K, m))
    for c in range(C_):
        for k in range(K):
            for j in range(m):
                q[c, k, j], inc[c, k, j] = proposal(lp[c, k, j], Pi[c, k])
    return q, inc


def min_log_ratio(lp):
    """The smallest lp - max_l lp: above about -700 no f_l underflows, and exp keeps its few-ulp error."""
    return float((lp - lp.max(axis=3, keepdims=True)).min())


def ulps(a, b):
    """|a - b| in units of the spacing at the larger magnitude."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class Mirror:
    """Step 4: the sums of everything added so far."""

    def __init__(self, K, m, n):
        self.K, self.m, self.n, self.T = K, m, n, 0
        self.sim = np.zeros((K, m, n), dtype=np.int64)
        self.new_cluster = np.zeros((K, m), dtype=np.int64)
        self.lpd_sum = np.zeros((K, m))

    def add(self, q, inc, s, empty):
        """q (C, K, m, N) integers, inc (C, K, m), s (C, K, n) 0-based labels (labels outside 0..N-1 add nothing), empty (C, K, N)."""
        C_, K, m, N = q.shape
        q = q.astype(np.int64)
        for c in range(C_):
            for k in range(K):
                ok = (s[c, k] >= 0) & (s[c, k] < N)
                lab = np.where(ok, s[c, k], 0)
                self.sim[k] += np.where(ok[None, :], q[c, k][:, lab], 0)
                self.new_cluster[k] += q[c, k][:, empty[c, k]].sum(axis=1)
        for k in range(K):
            for j in range(m):
                v = float(self.lpd_sum[k, j])
                for c in range(C_):
                    v = v + float(inc[c, k, j])
                self.lpd_sum[k, j] = v
        self.T += 1

    def merge(self, other):
        self.sim += other.sim
        self.new_cluster += other.new_cluster
        self.lpd_sum = self.lpd_sum + other.lpd_sum
        self.T += other.T

    def reset(self):
        self.__init__(self.K, self.m, self.n)

    def arrays(self):
        return {"sim": self.sim, "new_cluster": self.new_cluster, "lpd_sum": self.lpd_sum}
