"""Relabelling to a pivot: with what probability does observation i belong to cluster g?

align_labels! aligns the labels across the K datasets of one state, but every chain starts from a random allocation: label 3
of one chain and label 3 of another are different clusters, and anything indexed by label is meaningless once pooled over
chains.  The mixture-model answer is relabelling to a pivot (the assignment step of Stephens 2000; ECR of Papastamoulis &
Iliopoulos 2010): for every sampled state, the permutation of the N labels that agrees best with a fixed pivot clustering is
found exactly, applied, and the relabelled allocations are counted.  One permutation per state shared by all K datasets keeps
every event [c_a = c_b] intact, so the result stays consistent with Phi and fusion.FusionCounts.  RelabelAccumulator is the
streaming, device-resident form (include/pmdi_hip.h, pmdi_relabel_*); it ends in an AllocationProbabilities, a small host object
of numpy arrays.  The pivot may be known classes, a consensus clustering, DensityResult.best() of an earlier run, or the
result of a first pass (allocation_probabilities(iterate=...)).
"""
import ctypes as C

import numpy as np

from ._lib import _Accumulator, _check, _ptr, lib


def count_tile(N):
    """Observations per workgroup of the device's count kernel (a layout parameter, never a result parameter): the tests put
    n on both sides of it."""
    return 256 if int(N) <= 128 else 128


def as_pivot(pivot, K, n, N):
    """`pivot` as the (K, n) int32 array of pmdi_relabel_create: an (n,) integer array (the same for every dataset) or a
    (K, n) one, values 0..N-1, or -1 where the observation takes no part in the matching.  ValueError for anything else;
    needs no device."""
    a = np.asarray(pivot)
    K, n, N = int(K), int(n), int(N)
    if a.dtype.kind not in "iu" or a.ndim not in (1, 2):
        raise ValueError(f"the pivot must be an (n,) or (K, n) integer array, not {a.dtype} of shape {a.shape}")
    if a.shape[-1] != n or (a.ndim == 2 and a.shape[0] != K):
        raise ValueError(f"the pivot must be (n,) or (K, n) with K={K}, n={n}, not {a.shape}")
    if a.size and (int(a.min()) < -1 or int(a.max()) > N - 1):
        raise ValueError(f"pivot values must be 0..{N - 1}, or -1 where the observation takes no part in the matching")
    return np.ascontiguousarray(np.broadcast_to(a, (K, n)), dtype=np.int32)


class AllocationProbabilities:
    """What T retained draws of each of C chains say about the N components of the pivot, as plain numpy in the layouts of
    include/pmdi_hip.h (U = 1 unit per chain when the K datasets share one permutation, else U = K):
      alloc (K, n, N) int32        how often observation i of dataset k was drawn in component g, after relabelling
      match_sum (C, U) int64       (observation, dataset) pairs that agree with the pivot, summed over the draws
      moved (C, U) int64           draws whose permutation moves an occupied label
      w_sum, w_sq (C, K, N)        the relabelled mixture weights and their squares, summed over the draws; None without Pi
      n_match (U,) int64           (observation, dataset) pairs of a unit that take part in the matching (pivot >= 0)
    Built by RelabelAccumulator.result(), or directly from arrays."""

    def __init__(self, T, alloc, match_sum, moved, n_match, w_sum=None, w_sq=None, names=None):
        self.T = int(T)
        self.alloc = np.asarray(alloc, dtype=np.int32)
        if self.alloc.ndim != 3:
            raise ValueError(f"alloc must be (K, n, N), not {self.alloc.shape}")
        self.K, self.n, self.N = self.alloc.shape
        self.match_sum = np.asarray(match_sum, dtype=np.int64)
        if self.match_sum.ndim != 2 or self.match_sum.shape[1] not in (1, self.K):
            raise ValueError(f"match_sum must be (C, 1) or (C, K={self.K}), not {self.match_sum.shape}")
        self.C, self.U = self.match_sum.shape
        self.moved = np.asarray(moved, dtype=np.int64).reshape(self.C, self.U)
        self.n_match = np.asarray(n_match, dtype=np.int64).reshape(self.U)
        if (w_sum is None) != (w_sq is None):
            raise ValueError("w_sum and w_sq go together")
        self.w_sum = None if w_sum is None else np.asarray(w_sum, dtype=np.float64).reshape(self.C, self.K, self.N)
        self.w_sq = None if w_sq is None else np.asarray(w_sq, dtype=np.float64).reshape(self.C, self.K, self.N)
        self.names = list(names) if names is not None else [f"K{i}" for i in range(1, self.K + 1)]

    def _draws(self):
        if self.T < 1:
            raise ValueError("nothing was added yet")
        return self.C * self.T

    # ---- per observation ----
    def probabilities(self):
        """(K, n, N): the share of the C T draws in which observation i of dataset k sits in component g."""
        return self.alloc / float(self._draws())

    def hard(self):
        """(K, n) int32: the most probable component, ties to the smallest label."""
        self._draws()
        return np.argmax(self.alloc, axis=2).astype(np.int32)

    def confidence(self):
        """(K, n): the probability of hard()."""
        return self.alloc.max(axis=2) / float(self._draws())

    def entropy(self):
        """(K, n): the entropy of an observation's allocation probabilities, in bits (0 log 0 = 0)."""
        p = self.probabilities()
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(p > 0, p * np.log2(np.where(p > 0, p, 1.0)), 0.0)
        return -t.sum(axis=2) + 0.0

    def uncertain(self, level=0.8):
        """(K, n) bool: observations whose most probable component has less than `level`."""
        if not 0 < level <= 1:
            raise ValueError("uncertain: level must be in (0, 1]")
        return self.confidence() < level

    def expected_sizes(self):
        """(K, N): the posterior mean size of every component."""
        return self.alloc.sum(axis=1) / float(self._draws())

    def profiles(self, x, k):
        """(N, D): the soft cluster means of the data matrix x (n, D) of dataset k, P^T X / sum P with P = probabilities()[k];
        NaN for a component nothing was ever drawn in."""
        x = np.asarray(x, dtype=np.float64)
        if x.ndim != 2 or x.shape[0] != self.n or not 0 <= int(k) < self.K:
            raise ValueError(f"profiles: x must be (n={self.n}, D) and k in 0..{self.K - 1}")
        P = self.probabilities()[int(k)]
        tot = P.sum(axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(tot[:, None] > 0, (P.T @ x) / tot[:, None], np.nan)

    # ---- per component: the mixture weights ----
    def _need_weights(self):
        if self.w_sum is None:
            raise ValueError("no mixture weights were added (add_arrays without Pi)")
        return self._draws()

    def weights(self):
        """(K, N): the posterior mean of the mixture weight of every component, pooled over chains and draws."""
        draws = self._need_weights()
        return self.w_sum.sum(axis=0) / draws

    def weights_rhat(self):
        """(K, N): the classic Gelman-Rubin statistic of the relabelled weights over the C chains of T draws, in the convention
        of PosteriorSummary.rhat(): mean_c = w_sum / T, v_c = (w_sq - T mean_c^2) / (T - 1) (not below 0), W = mean_c v_c,
        B = T var_c(mean_c, ddof = 1), R-hat = sqrt((T - 1) / T + B / T / W); NaN where W = 0."""
        self._need_weights()
        if self.C < 2 or self.T < 2:
            raise ValueError(f"R-hat needs at least 2 chains of at least 2 draws (C={self.C}, T={self.T})")
        T = self.T
        mean = self.w_sum / T
        v = np.maximum(self.w_sq - T * mean * mean, 0.0) / (T - 1)
        W = v.sum(axis=0) / self.C
        B = T * np.var(mean, axis=0, ddof=1)
        out = np.full((self.K, self.N), np.nan)
        ok = W > 0
        out[ok] = np.sqrt((T - 1) / T + B[ok] / T / W[ok])
        return out

    # ---- per chain ----
    def agreement(self):
        """(C, U): the share of a chain's (observation, dataset) pairs that agree with the pivot after relabelling, averaged
        over its draws; a chain sitting in another mode stands out.  1 where nothing takes part in the matching."""
        self._draws()
        den = np.where(self.n_match > 0, self.T * self.n_match, 1).astype(np.float64)
        return np.where(self.n_match > 0, self.match_sum / den, 1.0)

    def switch_rate(self):
        """(U,): the share of the C T draws whose labels had to be permuted to match the pivot."""
        tot = np.array([sum(int(v) for v in self.moved[:, u]) for u in range(self.U)], dtype=np.float64)
        return tot / self._draws()

    def merge(self, other):
        """Pools the chains of another handle or GPU that were relabelled to the same pivot: alloc is added, the per-chain
        arrays are concatenated (self's first).  Needs the same T, shape, units and n_match; the weights are kept if both
        have them."""
        mine, theirs = (self.T, self.alloc.shape, self.U), (other.T, other.alloc.shape, other.U)
        if mine != theirs or not np.array_equal(self.n_match, other.n_match):
            raise ValueError(f"merge needs the same T, (K, n, N), units and n_match: {mine} vs {theirs}")
        cat = lambda name: np.concatenate([getattr(self, name), getattr(other, name)], axis=0)
        both = self.w_sum is not None and other.w_sum is not None
        return AllocationProbabilities(self.T, self.alloc + other.alloc, cat("match_sum"), cat("moved"), self.n_match,
                                       cat("w_sum") if both else None, cat("w_sq") if both else None, names=self.names)


class RelabelAccumulator(_Accumulator):
    """The streaming relabelling accumulator on one MI355X (include/pmdi_hip.h, pmdi_relabel_*): after every retained
    iteration it takes the device-resident allocations (and Pi) of every chain, forms the contingency table of the state
    against the pivot as an int8 matrix-core product, solves the N x N assignment problem exactly, one wavefront per (chain,
    unit), and counts the relabelled labels.  pivot: (n,) or (K, n) integers 0..N-1, -1 = takes no part in the matching.
    shared: one permutation per chain for all datasets (True), or one per dataset.  All calls go to the current torch stream of
    the device; use one stream per accumulator.  Everything is exact integers, the weights' sums bit-defined doubles."""
    _prefix = "pmdi_relabel"
    T = samples = property(_Accumulator._samples, doc="Adds so far = retained draws per chain.")

    def __init__(self, n_chains, K, N, n, pivot, shared=True, device=0):
        a = np.asarray(pivot)       # (shape errors here; the values are the library's to check)
        if a.dtype.kind not in "iu" or a.ndim not in (1, 2) or a.shape[-1] != int(n) or (a.ndim == 2 and a.shape[0] != int(K)):
            raise ValueError(f"pivot must be an (n,) or (K, n) integer array with K={int(K)}, n={int(n)}, not {a.dtype} of shape {a.shape}")
        self.pivot = np.ascontiguousarray(np.broadcast_to(np.clip(a, -2 ** 31, 2 ** 31 - 1), (int(K), int(n))), dtype=np.int32)
        h = C.c_void_p()
        _check(lib().pmdi_relabel_create(int(device), int(n_chains), int(K), int(N), int(n), _ptr(self.pivot), int(shared), C.byref(h)))
        self.h = h
        self.C, self.K, self.N, self.n, self.device = int(n_chains), int(K), int(N), int(n), int(device)
        self.shared = bool(shared)
        self.U = 1 if self.shared else self.K
        self._with_Pi = True         # until an add comes without Pi (add_gibbs and Gibbs.run always bring it)

    def set_pivot(self, pivot):
        """Another pivot, before the first add or after a reset (PmdiError(PMDI_E_STATE) otherwise)."""
        new = as_pivot(pivot, self.K, self.n, self.N)
        _check(lib().pmdi_relabel_set_pivot(self.h, _ptr(new), self._stream()))
        self.pivot = new

    def set_budget(self, nbytes):
        """Lowers the bytes of contingency tables one batch of chains may take; never changes a result."""
        _check(lib().pmdi_relabel_set_budget(self.h, int(nbytes)))

    def reset(self):
        super().reset()
        self._with_Pi = True

    def add_arrays(self, s, Pi=None):
        """s: CUDA int32 tensor (C, K, n) of 0-based labels, the layout of the resident state; Pi: CUDA float64 tensor
        (C, K, N) of the mixture weights, or None (the weights' sums are then left alone)."""
        import torch
        t = self._checked_tensor(s, torch.int32, (self.C, self.K, self.n), "add_arrays: s")
        w = None if Pi is None else self._checked_tensor(Pi, torch.float64, (self.C, self.K, self.N), "add_arrays: Pi")
        _check(lib().pmdi_relabel_add_arrays(self.h, C.c_void_p(t.data_ptr()), C.c_void_p(w.data_ptr()) if w is not None else None,
                                             self._stream()))
        self._with_Pi = self._with_Pi and Pi is not None

    def _empty(self):
        C_, K, N, U = self.C, self.K, self.N, self.U
        return {"alloc": np.zeros((K, self.n, N), dtype=np.int32), "match_sum": np.zeros((C_, U), dtype=np.int64),
                "moved": np.zeros((C_, U), dtype=np.int64), "w_sum": np.zeros((C_, K, N)), "w_sq": np.zeros((C_, K, N))}

    def arrays(self):
        """Host copies of every array of the accumulator (synchronises the stream); raises PmdiError(PMDI_E_DATA) if a label
        outside 0..N-1 was added since the last reset."""
        out = self._empty()
        _check(lib().pmdi_relabel_get(self.h, *[_ptr(a) for a in out.values()], self._stream()))
        return out

    def last(self):
        """(perm (C, U, N) uint8, value (C, U) int64) of the latest add (synchronises the stream)."""
        perm = np.zeros((self.C, self.U, self.N), dtype=np.uint8)
        value = np.zeros((self.C, self.U), dtype=np.int64)
        _check(lib().pmdi_relabel_last(self.h, _ptr(perm), _ptr(value), self._stream()))
        return perm, value

    def n_match(self):
        """(U,): the (observation, dataset) pairs of a unit that take part in the matching."""
        per = (self.pivot >= 0).sum(axis=1).astype(np.int64)
        return per.sum(keepdims=True) if self.shared else per

    def result(self, names=None):
        """The AllocationProbabilities of everything added so far; with the weights iff every add brought Pi."""
        a = self.arrays()
        if not self._with_Pi:
            a["w_sum"] = a["w_sq"] = None
        return AllocationProbabilities(self.T, n_match=self.n_match(), names=names, **a)


def allocation_probabilities(draws, pivot, N=None, shared=True, iterate=0, Pi=None, device=0):
    """Relabels resident draws afterwards -- the final states pmdi_pooled(final_allocations=True) returns are thousands of
    independent ones.  draws: (R, K, n) int32 of 0-based labels, a CUDA tensor or a numpy array; pivot: (n,) or (K, n); N: the
    number of labels (default: the largest label of draws and pivot + 1, at least 2); Pi: (R, K, N) float64 or None.
    iterate = m > 0: while hard() of the result differs from the pivot and fewer than m further passes were made, hard() becomes
    the pivot and the draws are relabelled again (a pivot entry of -1 never equals hard(), so such a pivot is replaced at least
    once).  Returns (AllocationProbabilities, info) with info = {"passes": relabelling passes made, "converged": hard() of the
    result equals the pivot it was matched to}."""
    import torch
    dev = torch.device("cuda", int(device))
    s = torch.as_tensor(draws)
    if s.dim() != 3 or s.dtype not in (torch.int32, torch.int64, torch.uint8):
        raise ValueError(f"draws must be an (R, K, n) integer array, not {s.dtype} {tuple(s.shape)}")
    if int(iterate) < 0:
        raise ValueError("iterate must be >= 0")
    R, K, n = (int(v) for v in s.shape)
    piv = np.asarray(pivot)
    if N is None:
        N = max(2, int(s.max()) + 1 if s.numel() else 2, int(piv.max()) + 1 if piv.size else 2)
    piv = as_pivot(piv, K, n, N)
    s = s.to(device=dev, dtype=torch.int32).contiguous()
    w = None if Pi is None else torch.as_tensor(Pi).to(device=dev, dtype=torch.float64).contiguous()
    acc = RelabelAccumulator(R, K, N, n, piv, shared=shared, device=device)
    try:
        passes = 0
        while True:
            acc.add_arrays(s, w)
            passes += 1
            res = acc.result()
            new = res.hard()
            converged = bool(np.array_equal(new, acc.pivot))
            if converged or passes > int(iterate):
                return res, {"passes": passes, "converged": converged}
            acc.reset()
            acc.set_pivot(new)
    finally:
        acc.close()


def assign_labels(tables, device=0):
    """The solver alone (pmdi_relabel_assign_device): tables (B, N, N) or (N, N) int32, a numpy array or a CUDA tensor, of any
    values; returns (perm (B, N) uint8, value (B,) int64) as numpy -- perm[b][l] = sigma(l) maximises sum_l tables[b][l][sigma(l)],
    the maximiser the pinned loop of include/pmdi_hip.h finds."""
    import torch
    dev = torch.device("cuda", int(device))
    t = torch.as_tensor(tables)
    if t.dim() == 2:
        t = t[None]
    if t.dim() != 3 or t.shape[1] != t.shape[2] or t.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"tables must be (B, N, N) or (N, N) integers, not {t.dtype} {tuple(t.shape)}")
    if t.numel() and (int(t.min()) < -2 ** 31 or int(t.max()) > 2 ** 31 - 1):
        raise ValueError("tables must hold int32 values")
    B, N = int(t.shape[0]), int(t.shape[1])
    t = t.to(device=dev, dtype=torch.int32).contiguous()
    perm = torch.zeros((B, N), dtype=torch.uint8, device=dev)
    value = torch.zeros((B,), dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream(dev)
    _check(lib().pmdi_relabel_assign_device(int(device), C.c_void_p(t.data_ptr()), B, N, C.c_void_p(perm.data_ptr()),
                                            C.c_void_p(value.data_ptr()), C.c_void_p(st.cuda_stream)))
    return perm.cpu().numpy(), value.cpu().numpy()
