"""The definitions behind the streaming summary accumulator (include/pmdi_hip.h, pmdi_summary_*), written out as plain
Python so that they can serve as its yardstick: len(np.unique(row)) for the cluster counts, a Python-float loop of the
three Welford lines, a Python loop over the chains for the trace.  Independent of the package's summary.py by design."""
import numpy as np


def nclust(s):
    """s (C, K, n) labels -> (C, K) int64: the number of distinct labels of every row."""
    s = np.asarray(s)
    return np.array([[len(np.unique(s[c, k])) for k in range(s.shape[1])] for c in range(s.shape[0])], dtype=np.int64)


class Mirror:
    """Every array of the accumulator, updated by definition.  Floats are Python floats (IEEE doubles, one rounding per
    operation, no fused multiply-add)."""

    def __init__(self, C, K, N, sumD=0, trace_cap=0):
        self.C, self.K, self.N, self.sumD, self.cap, self.T = C, K, N, sumD, trace_cap, 0
        self.P = K * (K - 1) // 2
        self.nclust_hist = np.zeros((K, N + 1), dtype=np.int64)
        self.nclust_sum = np.zeros((C, K), dtype=np.int64)
        self.nclust_sumsq = np.zeros((C, K), dtype=np.int64)
        self.M_mean = [[0.0] * K for _ in range(C)]
        self.M_m2 = [[0.0] * K for _ in range(C)]
        self.Phi_mean = [[0.0] * self.P for _ in range(C)]
        self.Phi_m2 = [[0.0] * self.P for _ in range(C)]
        self.flag_count = np.zeros(sumD, dtype=np.int64)
        self.trace_nclust, self.trace_M, self.trace_Phi = [], [], []

    @staticmethod
    def _welford(mean, m2, row, t):
        for j, x in enumerate(row):
            x = float(x)
            d = x - mean[j]
            mean[j] = mean[j] + d / t
            m2[j] = m2[j] + d * (x - mean[j])

    def add(self, s, M, Phi, flags=None):
        """s (C, K, n) 0-based labels, M (C, K), Phi (C, >= npairs), flags (C, sumD) or None."""
        self.T += 1
        t = float(self.T)
        m = nclust(s)
        for c in range(self.C):
            for k in range(self.K):
                self.nclust_hist[k, m[c, k]] += 1
            self._welford(self.M_mean[c], self.M_m2[c], M[c][:self.K], t)
            self._welford(self.Phi_mean[c], self.Phi_m2[c], Phi[c][:self.P], t)
        self.nclust_sum += m
        self.nclust_sumsq += m * m
        if flags is not None:
            self.flag_count += np.asarray(flags, dtype=np.int64).sum(axis=0)
        if self.T <= self.cap:
            self.trace_nclust.append([int(m[:, k].sum()) for k in range(self.K)])
            for rows, src, width in ((self.trace_M, M, self.K), (self.trace_Phi, Phi, self.P)):
                out = []
                for j in range(width):
                    acc = 0.0
                    for c in range(self.C):
                        acc = acc + float(src[c][j])
                    out.append(acc)
                rows.append(out)

    def arrays(self):
        f = lambda x, rows, w: np.array(x, dtype=np.float64).reshape(rows, w)
        C, K, P, R = self.C, self.K, self.P, len(self.trace_nclust)
        return {"nclust_hist": self.nclust_hist, "nclust_sum": self.nclust_sum, "nclust_sumsq": self.nclust_sumsq,
                "M_mean": f(self.M_mean, C, K), "M_m2": f(self.M_m2, C, K), "Phi_mean": f(self.Phi_mean, C, P),
                "Phi_m2": f(self.Phi_m2, C, P), "flag_count": self.flag_count,
                "trace_nclust": np.array(self.trace_nclust, dtype=np.int64).reshape(R, K),
                "trace_M": f(self.trace_M, R, K), "trace_Phi": f(self.trace_Phi, R, P)}


def same_bits(a, b):
    """Equality of float64 arrays bit for bit (or of integer arrays)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float64:
        return np.array_equal(a.view(np.int64), b.view(np.int64))
    return np.array_equal(a, b)


def rows_with_m_labels(rng, n, N, m, rare_at):
    """A row of n labels < N holding exactly min(m, n) distinct ones.  m = 1: all equal.  m = 2: one label everywhere but at
    position `rare_at`.  m = N (needs n >= N for N distinct ones): every label, each of the labels 1.. placed once at random
    positions except that the LAST label, N - 1, sits only at `rare_at`."""
    base = int(rng.integers(0, N))
    row = np.full(n, base, dtype=np.int32)
    if m == 1 or n == 1:
        return row, 1
    if m == 2:
        row[rare_at] = (base + 1) % N
        return row, 2
    if n < N:       # fewer places than labels: all different
        row[:] = rng.permutation(N)[:n]
        return row, n
    others = [p for p in range(n) if p != rare_at]
    row[:] = rng.integers(0, N - 1, size=n)                 # labels 0 .. N - 2 anywhere
    spots = rng.permutation(others)[:N - 1]
    row[spots] = np.arange(N - 1)                           # each of them at least once
    row[rare_at] = N - 1                                    # the rare one exactly once
    return row, N
