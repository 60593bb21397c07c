"""The definitions of the streaming agreement accumulator (include/pmdi_hip.h, pmdi_agreement_*) written out: the contingency
table with np.add.at, every integer a Python int, the adjusted Rand index and the sums of doubles as plain Python float loops
in the stated order.  The fixed-point logarithm takes its 2049 table entries from the caller (psm.vi_log2_table()).  Never the
package's own agreement.py."""
import math

import numpy as np

from _np_summary import same_bits  # noqa: F401    (equality bit for bit; the tests take it from here)

NAMES = ("both", "jl", "px", "py", "hx", "hy", "n_q")


def choose2(x):
    return int(x) * (int(x) - 1) // 2


def make_L(table):
    """L(x), 1 <= x < 2^62, in units of 2^-30 from the table T[k] = round(log2(1 + k / 2048) 2^30): Python integers only."""
    T = [int(v) for v in table]
    assert len(T) == 2049

    def L(x):
        x = int(x)
        assert 1 <= x < 2 ** 62
        e = x.bit_length() - 1
        f = (x << (62 - e)) - 2 ** 62
        k, r32 = f >> 51, (f & (2 ** 51 - 1)) >> 19
        return (e << 30) + T[k] + (((T[k + 1] - T[k]) * r32) >> 32)
    return L


def pairs_of(K):
    return [(a, b) for a in range(K) for b in range(a + 1, K)]


def table_of(x, y, Gx, Gy):
    """n_ab over the observations that count: x in 0..Gx-1 and y in 0..Gy-1 (a label outside, and the -1 of an unknown class,
    takes part in nothing -- the choice the device follows).  (Gx, Gy) int64."""
    x, y = np.asarray(x, dtype=np.int64), np.asarray(y, dtype=np.int64)
    ok = (x >= 0) & (x < Gx) & (y >= 0) & (y < Gy)
    t = np.zeros((Gx, Gy), dtype=np.int64)
    np.add.at(t, (x[ok], y[ok]), 1)
    return t


def integers(x, y, Gx, Gy, L):
    """(both, jl, px, py, hx, hy, n_q) of one comparison: the marginals are the row and column sums of the table."""
    t = table_of(x, y, Gx, Gy)
    sL = lambda v: v * L(v) if v > 0 else 0
    cells = [int(v) for v in t.reshape(-1) if v]
    rows, cols = [int(v) for v in t.sum(axis=1)], [int(v) for v in t.sum(axis=0)]
    return (sum(choose2(v) for v in cells), sum(sL(v) for v in cells), sum(choose2(v) for v in rows), sum(choose2(v) for v in cols),
            sum(sL(v) for v in rows), sum(sL(v) for v in cols), sum(cells))


def ari(both, px, py, T2):
    """The header's lines, one IEEE operation each."""
    if T2 == 0:
        return 1.0
    e = float(px) * float(py)
    e = e / float(T2)
    m = float(px) + float(py)
    m = m / 2.0
    den = m - e
    if den == 0.0:
        return 1.0
    num = float(both) - e
    return num / den


def hist_bin(a):
    return min(255, max(0, int(math.floor((a + 1.0) * 128.0))))


def brute_force(x, y):
    """(both, px, py, T2) by the loop over all pairs of the observations that count (y >= 0: the class is known)."""
    idx = [i for i in range(len(x)) if y[i] >= 0]
    both = px = py = T2 = 0
    for u in range(len(idx)):
        for v in range(u + 1, len(idx)):
            i, j = idx[u], idx[v]
            sx, sy = x[i] == x[j], y[i] == y[j]
            both += sx and sy
            px += sx
            py += sy
            T2 += 1
    return both, px, py, T2


class Mirror:
    """The accumulator on the host, one add at a time.  s (C, K, n) 0-based labels; ref (R, n) classes, -1 = unknown."""

    def __init__(self, C, K, N, n, ref, trace_cap, table):
        self.C, self.K, self.N, self.n, self.cap = C, K, N, n, trace_cap
        self.ref = np.zeros((0, n), dtype=np.int64) if ref is None else np.asarray(ref, dtype=np.int64).reshape(-1, n)
        self.R = self.ref.shape[0]
        self.G = K * (K - 1) // 2
        self.Q = self.G + self.R * K
        self.gr = [max(1, int(r.max()) + 1) for r in self.ref]
        self.L = make_L(table)
        self.reset()

    def reset(self):
        C, Q = self.C, self.Q
        self.T = 0
        self.rand_num = np.zeros((C, Q), dtype=np.int64)
        self.ari_sum = np.zeros((C, Q))
        self.ari_sq = np.zeros((C, Q))
        self.vi_sum = np.zeros((C, Q), dtype=np.int64)
        self.mi_sum = np.zeros((C, Q), dtype=np.int64)
        self.ari_hist = np.zeros((Q, 256), dtype=np.int64)
        self.trace = []
        self.last = np.zeros((C, Q, 7), dtype=np.int64)
        self.last_ari = None

    def sides(self, s_c, q):
        """(x, y, Gx, Gy) of comparison q of one chain's labels s_c (K, n)."""
        if q < self.G:
            a, b = pairs_of(self.K)[q]
            return s_c[a], s_c[b], self.N, self.N
        r, k = divmod(q - self.G, self.K)
        return s_c[k], self.ref[r], self.N, self.gr[r]

    def add(self, s):
        C, K, Q, L = self.C, self.K, self.Q, self.L
        s = np.asarray(s).reshape(C, K, self.n)
        aris = [[0.0] * Q for _ in range(C)]
        for c in range(C):
            for q in range(Q):
                both, jl, px, py, hx, hy, nq = v = integers(*self.sides(s[c], q), L)
                self.last[c, q] = v
                T2 = choose2(nq)
                self.rand_num[c, q] += T2 + 2 * both - px - py
                a = aris[c][q] = ari(both, px, py, T2)
                self.ari_sum[c, q] = float(self.ari_sum[c, q]) + a
                self.ari_sq[c, q] = float(self.ari_sq[c, q]) + a * a
                self.vi_sum[c, q] += hx + hy - 2 * jl
                self.mi_sum[c, q] += (nq * L(nq) if nq > 0 else 0) - hx - hy + jl
                self.ari_hist[q, hist_bin(a)] += 1
        if self.T < self.cap:
            row = []
            for q in range(Q):
                acc = 0.0
                for c in range(C):
                    acc = acc + aris[c][q]
                row.append(acc)
            self.trace.append(row)
        self.last_ari = aris
        self.T += 1

    def arrays(self):
        tr = np.zeros((self.cap, self.Q))
        if self.trace:
            tr[:len(self.trace)] = np.array(self.trace, dtype=np.float64)
        return {"rand_num": self.rand_num, "ari_sum": self.ari_sum, "ari_sq": self.ari_sq, "vi_sum": self.vi_sum,
                "mi_sum": self.mi_sum, "ari_hist": self.ari_hist, "trace": tr}
