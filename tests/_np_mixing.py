"""The definitions of the streaming mixing accumulator (include/pmdi_hip.h, pmdi_mixing_*) written out: the contingency table
with np.add.at on a * N + b, the pair counts in Python integers, the adjusted Rand index and the scalar recurrences as plain
Python float loops in the stated order.  Never the package's own mixing.py."""
import numpy as np

from _np_summary import same_bits  # noqa: F401    (equality bit for bit; the tests take it from here)


def choose2(x):
    return int(x) * (int(x) - 1) // 2


def marginal(row, N):
    """(P, occupied labels) of one row of labels: P = sum_a h_a (h_a - 1) / 2.  A label outside 0..N-1 is counted nowhere."""
    row = np.asarray(row, dtype=np.int64)
    ok = (row >= 0) & (row < N)
    h = np.bincount(row[ok], minlength=N)
    return sum(choose2(c) for c in h.tolist()), int((h > 0).sum())


def contingency_A(row, prev, N):
    """A = sum_ab n_ab (n_ab - 1) / 2 with n_ab = #{i: row_i = a, prev_i = b}, observations with a label outside 0..N-1 on
    either side counted nowhere."""
    row, prev = np.asarray(row, dtype=np.int64), np.asarray(prev, dtype=np.int64)
    ok = (row >= 0) & (row < N) & (prev >= 0) & (prev < N)
    table = np.zeros(N * N, dtype=np.int64)
    np.add.at(table, row[ok] * N + prev[ok], 1)
    return sum(choose2(c) for c in table.tolist() if c)


def agreeing_pairs(A, P, Q, n):
    return choose2(n) + 2 * A - P - Q


def ari(A, P, Q, n):
    """The header's lines, one IEEE operation each."""
    T2 = choose2(n)
    if T2 == 0:
        return 1.0
    e = float(P) * float(Q)
    e = e / float(T2)
    m = float(P) + float(Q)
    m = m / 2.0
    den = m - e
    if den == 0.0:
        return 1.0
    num = float(A) - e
    return num / den


def brute_force(row, prev):
    """(A, P, Q, agreeing pairs) by the loop over all pairs of observations."""
    n = len(row)
    A = P = Q = agree = 0
    for i in range(n):
        for j in range(i + 1, n):
            x, y = row[i] == row[j], prev[i] == prev[j]
            A += x and y
            P += x
            Q += y
            agree += x == y
    return A, P, Q, agree


class Mirror:
    """The accumulator on the host, one add at a time.  s (C, K, n) 0-based labels, M (C, K), Phi (C, max(1, npairs))."""

    def __init__(self, C, K, N, n, L):
        self.C, self.K, self.N, self.n, self.L = C, K, N, n, L
        self.npairs = K * (K - 1) // 2
        self.J = 2 * K + self.npairs
        self.reset()

    def reset(self):
        C, K, L, J = self.C, self.K, self.L, self.J
        self.T = 0
        self.rand_num = np.zeros((C, K, L), dtype=np.int64)
        self.ari_sum = np.zeros((C, K, L))
        self.sum_y = np.zeros((C, J))
        self.prod = np.zeros((C, J, L + 1))
        self.head = np.zeros((C, J, L))
        self.tail = np.zeros((C, J, L))
        self.first = np.zeros((C, J))
        self.samples, self.P, self.y = [], [], []            # the last L + 1 adds, newest last
        self.last_A = self.last_P = None

    def add(self, s, M, Phi):
        C, K, L, J, N, n = self.C, self.K, self.L, self.J, self.N, self.n
        s = np.asarray(s).reshape(C, K, n)
        t = self.T + 1
        P = [[0] * K for _ in range(C)]
        x = [[0.0] * J for _ in range(C)]
        for c in range(C):
            for k in range(K):
                P[c][k], occupied = marginal(s[c, k], N)
                x[c][k] = float(M[c][k])
                x[c][K + self.npairs + k] = float(occupied)
            for p in range(self.npairs):
                x[c][K + p] = float(Phi[c][p])
        nl = min(L, t - 1)
        self.last_A = np.zeros((C, K, L), dtype=np.int64)
        for c in range(C):
            for k in range(K):
                for lag in range(1, nl + 1):
                    prev, Q = self.samples[-lag][c, k], self.P[-lag][c][k]
                    A = contingency_A(s[c, k], prev, N)
                    self.last_A[c, k, lag - 1] = A
                    self.rand_num[c, k, lag - 1] += agreeing_pairs(A, P[c][k], Q, n)
                    self.ari_sum[c, k, lag - 1] = float(self.ari_sum[c, k, lag - 1]) + ari(A, P[c][k], Q, n)
        y = [[0.0] * J for _ in range(C)]
        for c in range(C):
            for j in range(J):
                if t == 1:
                    self.first[c, j] = x[c][j]
                y[c][j] = x[c][j] - float(self.first[c, j])
        self.samples.append(s.copy()); self.P.append(P); self.y.append(y)
        for lst in (self.samples, self.P, self.y):
            del lst[:-(L + 1)]
        for c in range(C):
            for j in range(J):
                yt = y[c][j]
                self.sum_y[c, j] = float(self.sum_y[c, j]) + yt
                for lag in range(0, nl + 1):
                    p = yt * self.y[-1 - lag][c][j]
                    self.prod[c, j, lag] = float(self.prod[c, j, lag]) + p
                if t <= L:
                    self.head[c, j, t - 1] = yt
                for i in range(L):
                    back = L - 1 - i
                    self.tail[c, j, i] = self.y[-1 - back][c][j] if back < t else 0.0
        self.last_P = P
        self.T = t

    def arrays(self):
        return {"rand_num": self.rand_num, "ari_sum": self.ari_sum, "sum_y": self.sum_y, "prod": self.prod, "head": self.head,
                "tail": self.tail, "first": self.first}
