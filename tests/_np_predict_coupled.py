"""The yardstick of the coupled add of the predictive accumulator (include/pmdi_hip.h, "coupled add"): a plain Python float-loop
mirror of its steps 1-7 in the stated order, a brute-force enumeration of all N^K label tuples to hold the mirror to, and a Mirror
of the four joint sums.  TEST INFRASTRUCTURE ONLY."""
import itertools
import math

import numpy as np

Q_ONE = 1 << 20
DBL_MAX = 1.7976931348623157e308


def pairs(K):
    """Phi's own pair order."""
    return [(a, b) for a in range(K - 1) for b in range(a + 1, K)]


def fill_W(K, Phi):
    W = [[0.0] * 8 for _ in range(8)]
    for i, (a, b) in enumerate(pairs(K)):
        W[a][b] = W[b][a] = float(Phi[i])
    return W


def _subsets(active):
    """The non-empty subsets of `active` in ascending mask order."""
    B = (0 - active) & active
    while B:
        yield B
        B = (B - active) & active


def conn_all(active, W):
    conn = {}
    for B in _subsets(active):
        v = (B & -B).bit_length() - 1
        R = B & (B - 1)
        if R == 0:
            conn[B] = 1.0
            continue
        link = {0: 0.0}
        for C in _subsets(R):
            hb = C.bit_length() - 1
            w, r = W[v][hb], link[C ^ (1 << hb)]
            link[C] = r + w + r * w
        F = {0: 1.0}
        for S in _subsets(R):
            low = S & -S
            Sp = S ^ low
            acc, Cp = 0.0, 0
            while True:
                Cc = Cp | low
                acc += conn[Cc] * link[Cc] * F[Sp ^ Cp]
                Cp = (Cp - Sp) & Sp
                if Cp == 0:
                    break
            F[S] = acc
        conn[B] = F[R]
    return conn


def zs_all(active, conn, T):
    Zs = {0: 1.0}
    for S in _subsets(active):
        low = S & -S
        Sp = S ^ low
        acc, Cp = 0.0, 0
        while True:
            B = Cp | low
            acc += conn[B] * T[B] * Zs[Sp ^ Cp]
            Cp = (Cp - Sp) & Sp
            if Cp == 0:
                break
        Zs[S] = acc
    return Zs


def compute_T(K, N, g):
    T = {}
    for B in range(1, 1 << K):
        acc = 0.0
        for l in range(N):
            p = 1.0
            for k in range(K):
                if B >> k & 1:
                    p = p * g[k][l]
            acc += p
        T[B] = acc
    return T


def chain_tables(K, Phi):
    """What depends on the chain only: (W, conn, [conn2 of every pair])."""
    full = (1 << K) - 1
    W = fill_W(K, Phi)
    conn2 = []
    for a, b in pairs(K):
        W2 = [row[:] for row in W]
        for u in range(K):
            if u in (a, b):
                continue
            wa, wb = W[a][u], W[b][u]
            W2[a][u] = W2[u][a] = wa + wb + wa * wb
        conn2.append(conn_all(full ^ (1 << b), W2))
    return W, conn_all(full, W), conn2


def recursion(K, N, g, Phi, tables=None):
    """Steps 2-5 for one (chain, new row) from g (K lists of N floats): (Z, S [K][N], R [G])."""
    g = [[float(v) for v in row] for row in g]
    _, conn, conn2 = tables if tables is not None else chain_tables(K, Phi)
    full = (1 << K) - 1
    T = compute_T(K, N, g)
    Zs = zs_all(full, conn, T)
    Z = Zs[full]
    S = [[0.0] * N for _ in range(K)]
    for k in range(K):
        U = full ^ (1 << k)
        for l in range(N):
            acc, Cq = 0.0, 0
            while True:
                B = Cq | (1 << k)
                p = 1.0
                for u in range(K):
                    if B >> u & 1:
                        p = p * g[u][l]
                acc += conn[B] * p * Zs[U ^ Cq]
                Cq = (Cq - U) & U
                if Cq == 0:
                    break
            S[k][l] = acc
    R = []
    for i, (a, b) in enumerate(pairs(K)):
        rest = full ^ (1 << a) ^ (1 << b)
        acc, Cq = 0.0, 0
        while True:
            acc += conn2[i][Cq | (1 << a)] * T[Cq | (1 << a) | (1 << b)] * Zs[rest ^ Cq]
            Cq = (Cq - rest) & rest
            if Cq == 0:
                break
        R.append(acc * (1.0 + float(Phi[i])))
    return Z, S, R


def fixed(w):
    return int(math.floor(w * 1048576.0 + 0.5))


def quantise(Z, S, R):
    """Steps 4, 5 and 7: (qj [K][N], fq [G]) as Python ints."""
    if not (Z > 0.0 and Z <= DBL_MAX):
        return [[0] * len(row) for row in S], [0] * len(R)
    return [[fixed(v / Z) for v in row] for row in S], [fixed(v / Z) for v in R]


def weights(lp_rows, Pi_rows):
    """Step 1 for one (chain, new row): (g [K][N], mx [K]) from lp [K][N] and Pi [K][N]."""
    g, mx = [], []
    for lp, Pi in zip(lp_rows, Pi_rows):
        lp = [float(v) for v in lp]
        top = max(lp)
        mx.append(top)
        g.append([math.exp(v - top) * float(p) for v, p in zip(lp, Pi)])
    return g, mx


def sum_mx(mx):
    v = mx[0]
    for x in mx[1:]:
        v = v + x
    return v


def brute_force(K, N, g, Phi):
    """The same three things over all N^K label tuples (math.fsum: exactly rounded sums of the tuples' weights)."""
    pr = pairs(K)
    terms, S_terms, R_terms = [], [[[] for _ in range(N)] for _ in range(K)], [[] for _ in pr]
    for c in itertools.product(range(N), repeat=K):
        w = 1.0
        for k in range(K):
            w *= float(g[k][c[k]])
        for i, (a, b) in enumerate(pr):
            if c[a] == c[b]:
                w *= 1.0 + float(Phi[i])
        terms.append(w)
        for k in range(K):
            S_terms[k][c[k]].append(w)
        for i, (a, b) in enumerate(pr):
            if c[a] == c[b]:
                R_terms[i].append(w)
    return math.fsum(terms), [[math.fsum(t) for t in row] for row in S_terms], [math.fsum(t) for t in R_terms]


def couple_all(g, Phi, Pi, mx):
    """Steps 2-7 everywhere from g (C, K, m, N), Phi (C, G), Pi (C, K, N) and mx (C, K, m): a dict of Z (C, m), Z0 (C,),
    qj (C, K, m, N) int64, fq (C, G, m) int64, incj (C, m) and the three magnitudes incj is formed from."""
    C_, K, m, N = g.shape
    G = K * (K - 1) // 2
    out = {"Z": np.zeros((C_, m)), "Z0": np.zeros(C_), "qj": np.zeros((C_, K, m, N), dtype=np.int64),
           "fq": np.zeros((C_, G, m), dtype=np.int64), "incj": np.zeros((C_, m)), "scale": np.zeros((C_, m))}
    for c in range(C_):
        tables = chain_tables(K, Phi[c])
        Z0, _, _ = recursion(K, N, Pi[c], Phi[c], tables)
        out["Z0"][c] = Z0
        for j in range(m):
            Z, S, R = recursion(K, N, g[c, :, j, :], Phi[c], tables)
            qj, fq = quantise(Z, S, R)
            out["Z"][c, j] = Z
            out["qj"][c, :, j, :] = qj
            out["fq"][c, :, j] = fq
            smx = sum_mx([float(v) for v in mx[c, :, j]])
            out["incj"][c, j] = (math.log(Z) - math.log(Z0)) + smx
            out["scale"][c, j] = max(abs(math.log(Z)), abs(math.log(Z0)), abs(smx))
    return out


class Mirror:
    """The four joint sums of everything added so far."""

    def __init__(self, K, m, n):
        self.K, self.m, self.n, self.T = K, m, n, 0
        G = K * (K - 1) // 2
        self.sim_joint = np.zeros((K, m, n), dtype=np.int64)
        self.new_cluster_joint = np.zeros((K, m), dtype=np.int64)
        self.fused_new = np.zeros((G, m), dtype=np.int64)
        self.lpd_joint_sum = np.zeros(m)

    def add(self, qj, fq, incj, s, empty):
        """qj (C, K, m, N), fq (C, G, m) integers, incj (C, m), s (C, K, n) 0-based labels (labels outside 0..N-1 add nothing),
        empty (C, K, N) bool."""
        C_, K, m, N = qj.shape
        qj = qj.astype(np.int64)
        for c in range(C_):
            for k in range(K):
                ok = (s[c, k] >= 0) & (s[c, k] < N)
                lab = np.where(ok, s[c, k], 0)
                self.sim_joint[k] += np.where(ok[None, :], qj[c, k][:, lab], 0)
                self.new_cluster_joint[k] += qj[c, k][:, empty[c, k]].sum(axis=1)
            self.fused_new += fq[c].astype(np.int64)
        for j in range(m):
            v = float(self.lpd_joint_sum[j])
            for c in range(C_):
                v = v + float(incj[c, j])
            self.lpd_joint_sum[j] = v
        self.T += 1

    def merge(self, other):
        self.sim_joint += other.sim_joint
        self.new_cluster_joint += other.new_cluster_joint
        self.fused_new += other.fused_new
        self.lpd_joint_sum = self.lpd_joint_sum + other.lpd_joint_sum
        self.T += other.T

    def reset(self):
        self.__init__(self.K, self.m, self.n)

    def arrays(self):
        return {"sim_joint": self.sim_joint, "new_cluster_joint": self.new_cluster_joint, "fused_new": self.fused_new,
                "lpd_joint_sum": self.lpd_joint_sum}
