"""The yardstick of the relabelling accumulator (include/pmdi_hip.h, pmdi_relabel_*): the contingency tables by np.add.at, the
assignment loop of the header in Python ints, the scatter into alloc and the sums of doubles as Python loops in the stated
order.  assign_np is the same loop with its column scans in numpy int64, for the large matrices of the GPU tests;
tests/test_relabel_host.py holds the two equal.  No device, no library."""
import numpy as np


def tables_of(s, pivot, N, shared):
    """(C, U, N, N) int64: W[c][u][l][g] over the datasets of unit u; a label outside 0..N-1 and a pivot of -1 are in no cell."""
    s, pivot = np.asarray(s), np.asarray(pivot)
    C_, K, n = s.shape
    U = 1 if shared else K
    W = np.zeros((C_, U, N, N), dtype=np.int64)
    for c in range(C_):
        for k in range(K):
            ok = (s[c, k] >= 0) & (s[c, k] < N) & (pivot[k] >= 0)
            np.add.at(W[c, 0 if shared else k], (s[c, k][ok], pivot[k][ok]), 1)
    return W


def assign(W):
    """(sigma, value): the pinned loop on an N x N matrix of Python ints (any integers)."""
    W = [[int(x) for x in row] for row in W]
    N = len(W)
    u, v = [0] * (N + 1), [0] * (N + 1)
    p, way = [-1] * (N + 1), [0] * (N + 1)
    for i in range(N):
        p[N] = i
        j0 = N
        minv = [None] * N                   # None = +infinity
        used = [False] * (N + 1)
        while p[j0] != -1:
            used[j0] = True
            i0 = p[j0]
            for j in range(N):
                if not used[j]:
                    cur = -W[i0][j] - u[i0] - v[j]
                    if minv[j] is None or cur < minv[j]:
                        minv[j], way[j] = cur, j0
            delta, j1 = None, -1
            for j in range(N):
                if not used[j] and (delta is None or minv[j] < delta):
                    delta, j1 = minv[j], j
            for j in range(N + 1):
                if used[j]:
                    u[p[j]] += delta
                    v[j] -= delta
                elif j < N:
                    minv[j] -= delta
            j0 = j1
        while j0 != N:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    sigma = [0] * N
    for j in range(N):
        sigma[p[j]] = j
    return sigma, sum(W[l][sigma[l]] for l in range(N))


class Mirror:
    """The accumulator's state after the same adds."""

    def __init__(self, C_, K, N, n, pivot, shared):
        self.C, self.K, self.N, self.n, self.shared = C_, K, N, n, bool(shared)
        self.U = 1 if shared else K
        self.pivot = np.broadcast_to(np.asarray(pivot), (K, n)).copy()
        self.reset()

    def reset(self):
        C_, K, N, n, U = self.C, self.K, self.N, self.n, self.U
        self.T = 0
        self.alloc = np.zeros((K, n, N), dtype=np.int32)
        self.match_sum = np.zeros((C_, U), dtype=np.int64)
        self.moved = np.zeros((C_, U), dtype=np.int64)
        self.w_sum = np.zeros((C_, K, N))
        self.w_sq = np.zeros((C_, K, N))
        self.perm = np.zeros((C_, U, N), dtype=np.uint8)
        self.value = np.zeros((C_, U), dtype=np.int64)

    def add(self, s, Pi=None):
        s = np.asarray(s)
        N = self.N
        W = tables_of(s, self.pivot, N, self.shared)
        for c in range(self.C):
            for u in range(self.U):
                sigma, value = (assign if N <= 64 else assign_np)(W[c, u])      # (the same loop: the scans in numpy beyond 64 labels)
                self.perm[c, u], self.value[c, u] = sigma, value
                self.match_sum[c, u] += value
                self.moved[c, u] += int(any(W[c, u, l].any() and sigma[l] != l for l in range(N)))
            for k in range(self.K):
                sigma = self.perm[c, 0 if self.shared else k]
                for i in range(self.n):
                    l = int(s[c, k, i])
                    if 0 <= l < N:
                        self.alloc[k, i, sigma[l]] += 1
                if Pi is not None:
                    for l in range(N):
                        x = float(Pi[c, k, l])
                        g = int(sigma[l])
                        self.w_sum[c, k, g] = self.w_sum[c, k, g] + x
                        self.w_sq[c, k, g] = self.w_sq[c, k, g] + x * x
        self.T += 1

    def arrays(self):
        return {"alloc": self.alloc, "match_sum": self.match_sum, "moved": self.moved, "w_sum": self.w_sum, "w_sq": self.w_sq}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def matrix_families(rng, N):
    """The five families of matrices the solver is tested on, by name."""
    perm = rng.permutation(N)
    z = rng.integers(0, N, 40 * N)
    noisy = np.zeros((N, N), dtype=np.int64)
    y = np.where(rng.random(z.size) < 0.2, rng.integers(0, N, z.size), perm[z])
    np.add.at(noisy, (z, y), 1)
    return {"ties": rng.integers(0, 3, (N, N)), "zero": np.zeros((N, N), dtype=np.int64),
            "large": rng.integers(0, 524281, (N, N)), "negative": rng.integers(-5, 5, (N, N)), "noisy": noisy}


def assign_np(W):
    """The same loop with the scans over the columns as numpy int64 operations (exact: |W| < 2^31 and the potentials stay far
    below 2^62); argmin returns the first minimum, the smallest j.  tests/test_relabel_host.py holds it equal to assign()."""
    W = np.asarray(W, dtype=np.int64)
    N = W.shape[0]
    INF = np.iinfo(np.int64).max
    u, v = np.zeros(N + 1, dtype=np.int64), np.zeros(N + 1, dtype=np.int64)
    p, way = np.full(N + 1, -1, dtype=np.int64), np.zeros(N + 1, dtype=np.int64)
    for i in range(N):
        p[N] = i
        j0 = N
        minv = np.full(N, INF, dtype=np.int64)
        used = np.zeros(N + 1, dtype=bool)
        while p[j0] != -1:
            used[j0] = True
            i0 = p[j0]
            free = ~used[:N]
            cur = -W[i0] - u[i0] - v[:N]
            upd = free & (cur < minv)
            minv[upd] = cur[upd]
            way[:N][upd] = j0
            m = np.where(free, minv, INF)
            j1 = int(np.argmin(m))
            delta = m[j1]
            uj = np.nonzero(used)[0]
            u[p[uj]] += delta
            v[uj] -= delta
            minv[free] -= delta
            j0 = j1
        while j0 != N:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    sigma = np.zeros(N, dtype=np.int64)
    sigma[p[:N]] = np.arange(N)
    return sigma.tolist(), int(W[np.arange(N), sigma].sum())
