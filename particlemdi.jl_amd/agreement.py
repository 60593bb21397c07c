"""Agreement between clusterings: the adjusted Rand index across datasets and against known classes, from a pooled run.

Phi_ab is a parameter of the prior; whether datasets a and b share their structure is read off it only indirectly, and
fusion.FusionCounts counts equal *labels*, which depends on the labels having been matched.  The label-free measure is the
adjusted Rand index (ARI) between the two clusterings of one sampled state; the standard figure of an applied analysis is the
ARI of every dataset's clustering with classes known in advance (tumour subtype, tissue), usually for a part of the
observations only.  A pooled run keeps no samples, so AgreementAccumulator is the streaming, device-resident form
(include/pmdi_hip.h, pmdi_agreement_*): after every retained iteration it forms the contingency table of every comparison of
every chain on the MI355X and keeps the sums.  It ends in an AgreementSummary, a small host object of numpy arrays.
"""
import numpy as np

from ._lib import _Accumulator, _check, _ptr, lib

MAX_REFERENCES = 8


def as_references(ref, n):
    """`ref` as the (R, n) int32 array of pmdi_agreement_create: None -> (0, n); an (n,) or (R, n) integer array (R <= 8)
    of classes 0..254 with -1 = unknown.  ValueError for anything else; needs no device."""
    if ref is None:
        return np.zeros((0, int(n)), dtype=np.int32)
    a = np.asarray(ref)
    if a.dtype.kind not in "iu" or a.ndim not in (1, 2):
        raise ValueError(f"reference labellings must be an (n,) or (R, n) integer array, not {a.dtype} of shape {a.shape}")
    a = a.reshape(1, -1) if a.ndim == 1 else a
    if a.shape[1] != int(n) or not 1 <= a.shape[0] <= MAX_REFERENCES:
        raise ValueError(f"reference labellings must be (n,) or (R, n) with n={int(n)} and 1 <= R <= {MAX_REFERENCES}, not {a.shape}")
    if a.size and (int(a.min()) < -1 or int(a.max()) > 254):
        raise ValueError("reference classes must be 0..254, or -1 where the class is unknown")
    return np.ascontiguousarray(a, dtype=np.int32)


class AgreementSummary:
    """What T retained draws of each of C chains say about Q = G + R K comparisons (K datasets, G = K (K - 1) / 2 pairs (a < b)
    in the order of Phi, then comparison G + r K + k = dataset k against reference r), as plain numpy in the layouts of
    include/pmdi_hip.h:
      rand_num (C, Q) int64     pairs of observations on which the two sides agree, summed over the draws
      ari_sum, ari_sq (C, Q)    the adjusted Rand index and its square, summed over the draws
      vi_sum, mi_sum (C, Q) int64   n_q times the variation of information / the mutual information in bits, times 2^30
      ari_hist (Q, 256) int64   draws of all chains by floor((ari + 1) 128), clamped to 0..255
      trace (rows, Q) or None   per retained iteration the sum of the ARI over the chains
      n_q (Q,) int64            observations that count in a comparison: n for a pair, the labelled ones for a reference
    Built by AgreementAccumulator.result(), or directly from arrays."""

    def __init__(self, T, K, n_q, rand_num, ari_sum, ari_sq, vi_sum, mi_sum, ari_hist, trace=None, names=None):
        self.T, self.K = int(T), int(K)
        self.rand_num = np.asarray(rand_num, dtype=np.int64)
        if self.rand_num.ndim != 2:
            raise ValueError(f"rand_num must be (C, Q), not {self.rand_num.shape}")
        self.C, self.Q = self.rand_num.shape
        self.G = self.K * (self.K - 1) // 2
        if self.Q < self.G or (self.Q - self.G) % self.K:
            raise ValueError(f"Q={self.Q} comparisons are not G + R K for K={self.K}")
        self.R = (self.Q - self.G) // self.K
        C_, Q = self.C, self.Q
        self.n_q = np.asarray(n_q, dtype=np.int64).reshape(Q)
        self.ari_sum = np.asarray(ari_sum, dtype=np.float64).reshape(C_, Q)
        self.ari_sq = np.asarray(ari_sq, dtype=np.float64).reshape(C_, Q)
        self.vi_sum = np.asarray(vi_sum, dtype=np.int64).reshape(C_, Q)
        self.mi_sum = np.asarray(mi_sum, dtype=np.int64).reshape(C_, Q)
        self.ari_hist = np.asarray(ari_hist, dtype=np.int64).reshape(Q, 256)
        self._trace = None if trace is None else np.asarray(trace, dtype=np.float64).reshape(-1, Q)
        self.names = list(names) if names is not None else [f"K{i}" for i in range(1, self.K + 1)]

    @property
    def comparisons(self):
        """The Q comparisons in order: (a, b) for a pair of datasets, (k, "ref r") for dataset k against reference r."""
        K = self.K
        return [(a, b) for a in range(K) for b in range(a + 1, K)] + [(k, f"ref {r}") for r in range(self.R) for k in range(K)]

    def _draws(self):
        if self.T < 1:
            raise ValueError("nothing was added yet")
        return self.C * self.T

    # ---- pooled means ----
    def ari(self):
        """(Q,): the posterior mean of the adjusted Rand index, pooled over chains and draws."""
        return self.ari_sum.sum(axis=0) / self._draws()

    def ari_matrix(self):
        """(K, K), symmetric with a NaN diagonal: ari() of the dataset pairs, to set beside PosteriorSummary.phi_matrix()."""
        m = np.full((self.K, self.K), np.nan)
        a = self.ari()
        for q, (i, j) in enumerate(self.comparisons[:self.G]):
            m[i, j] = m[j, i] = a[q]
        return m

    def _ref_slice(self, r):
        if not 0 <= int(r) < self.R:
            raise ValueError(f"reference {r} is not in 0..{self.R - 1}")
        return slice(self.G + int(r) * self.K, self.G + (int(r) + 1) * self.K)

    def against(self, r=0):
        """(K,): the posterior mean ARI of every dataset's clustering with reference labelling r."""
        return self.ari()[self._ref_slice(r)]

    def rand(self):
        """(Q,): the mean (unadjusted) Rand index, exact integers divided once; 1 where fewer than two observations count."""
        T2 = self.n_q * (self.n_q - 1) // 2
        tot = np.array([sum(int(v) for v in self.rand_num[:, q]) for q in range(self.Q)], dtype=np.float64)
        return np.where(T2 > 0, tot / np.where(T2 > 0, self._draws() * T2, 1), 1.0)

    def _bits(self, sums):
        tot = np.array([sum(int(v) for v in sums[:, q]) for q in range(self.Q)], dtype=np.float64)
        return np.where(self.n_q > 0, tot / np.where(self.n_q > 0, self._draws() * self.n_q * 2.0 ** 30, 1), 0.0)

    def vi(self):
        """(Q,): the mean variation of information between the two sides, in bits (fixed-point log2: include/pmdi_hip.h)."""
        return self._bits(self.vi_sum)

    def mi(self):
        """(Q,): the mean mutual information between the two sides, in bits."""
        return self._bits(self.mi_sum)

    # ---- per chain ----
    def chain_ari(self):
        """(C, Q): every chain's mean ARI."""
        self._draws()
        return self.ari_sum / self.T

    def _need_chains(self, what):
        if self.C < 2 or self.T < 2:
            raise ValueError(f"{what} needs at least 2 chains of at least 2 draws (C={self.C}, T={self.T})")

    def rhat(self):
        """(Q,): the classic Gelman-Rubin statistic of the ARI over the C chains of T draws, in the convention of
        PosteriorSummary.rhat(): mean_c = ari_sum / T, v_c = (ari_sq - T mean_c^2) / (T - 1) (not below 0), W = mean_c v_c,
        B = T var_c(mean_c, ddof = 1), R-hat = sqrt((T - 1) / T + B / T / W); NaN where W = 0."""
        self._need_chains("R-hat")
        T = self.T
        mean = self.ari_sum / T
        v = np.maximum(self.ari_sq - T * mean * mean, 0.0) / (T - 1)
        W = v.sum(axis=0) / self.C
        B = T * np.var(mean, axis=0, ddof=1)
        out = np.full(self.Q, np.nan)
        ok = W > 0
        out[ok] = np.sqrt((T - 1) / T + B[ok] / T / W[ok])
        return out

    def mcse(self):
        """(Q,): the between-chain standard error of ari(): sqrt(var_c(chain mean, ddof = 1) / C)."""
        if self.C < 2:
            raise ValueError("the between-chain standard error needs at least 2 chains")
        return np.sqrt(np.var(self.chain_ari(), axis=0, ddof=1) / self.C)

    # ---- the histogram ----
    def quantiles(self, p):
        """(Q,) for a scalar p, (len(p), Q) otherwise: quantiles of the ARI over all draws of all chains, from ari_hist.  Bin b
        holds the draws with b / 128 - 1 <= ari < (b + 1) / 128 - 1 (bin 255 also ari = 1): the edges are exact multiples of
        1 / 128, and a quantile is resolved no finer than that.  With S draws and cum_b the draws in the bins up to b, the
        p-quantile lies in the first occupied bin b with cum_b >= p S, at its lower edge plus (p S - cum_{b-1}) / count_b of
        its width: p S = cum_b gives the bin's upper edge exactly, p = 0 the lower edge of the lowest occupied bin."""
        ps = np.atleast_1d(np.asarray(p, dtype=np.float64))
        if ((ps < 0) | (ps > 1)).any():
            raise ValueError("quantiles: p must be in 0..1")
        out = np.full((len(ps), self.Q), np.nan)
        for q in range(self.Q):
            cnt = [int(v) for v in self.ari_hist[q]]
            S = sum(cnt)
            if S == 0:
                continue
            for j, pj in enumerate(ps):
                target, before = float(pj) * S, 0
                for b in range(256):
                    if cnt[b] and before + cnt[b] >= target:
                        out[j, q] = (b + (target - before) / cnt[b]) / 128.0 - 1.0
                        break
                    before += cnt[b]
        return out[0] if np.ndim(p) == 0 else out

    def interval(self, level=0.95):
        """(lower, upper), each (Q,): the central credible interval of the ARI at `level`, quantiles((1 -+ level) / 2)."""
        if not 0 < level < 1:
            raise ValueError("interval: level must be in (0, 1)")
        lo, hi = self.quantiles([(1.0 - level) / 2.0, (1.0 + level) / 2.0])
        return lo, hi

    def trace(self):
        """(rows, Q): per retained iteration the ARI averaged over the chains; None without a trace."""
        return None if self._trace is None else self._trace / self.C

    def merge(self, other):
        """Pools the chains of another handle or GPU: per-chain arrays are concatenated (self's first), the histograms added,
        the trace rows added (kept only if both have the same number).  Needs the same T, K, Q and n_q."""
        mine, theirs = (self.T, self.K, self.Q), (other.T, other.K, other.Q)
        if mine != theirs or not np.array_equal(self.n_q, other.n_q):
            raise ValueError(f"merge needs the same T, K, Q and n_q: {mine} {self.n_q.tolist()} vs {theirs} {other.n_q.tolist()}")
        cat = lambda name: np.concatenate([getattr(self, name), getattr(other, name)], axis=0)
        tr = None
        if self._trace is not None and other._trace is not None and self._trace.shape == other._trace.shape:
            tr = self._trace + other._trace
        return AgreementSummary(self.T, self.K, self.n_q, *[cat(x) for x in ("rand_num", "ari_sum", "ari_sq", "vi_sum", "mi_sum")],
                                self.ari_hist + other.ari_hist, tr, names=self.names)


class AgreementAccumulator(_Accumulator):
    """The streaming agreement accumulator on one MI355X (include/pmdi_hip.h, pmdi_agreement_*): after every retained
    iteration it takes the device-resident allocations of every chain and adds, per chain and comparison, the adjusted Rand
    index, its square, the agreeing pairs and the fixed-point variation of information and mutual information; the contingency
    tables are int8 matrix-core products and never leave the registers.  ref: None, or an (n,) or (R, n) integer array of known
    classes 0..254, -1 where unknown (as_references).  trace_cap: rows of the trace.  All calls go to the current torch stream
    of the device; use one stream per accumulator.  The integers are exact; the doubles are bit-defined by the order of the adds
    (the header states every operation)."""
    _prefix = "pmdi_agreement"
    T = samples = property(_Accumulator._samples, doc="Adds so far = retained draws per chain.")

    def __init__(self, n_chains, K, N, n, ref=None, trace_cap=0, device=0):
        import ctypes as C
        if ref is None:
            self.ref = np.zeros((0, max(int(n), 0)), dtype=np.int32)
        else:       # (shape errors here; the values and R are the library's to check)
            a = np.asarray(ref)
            if a.dtype.kind not in "iu" or a.ndim not in (1, 2) or a.shape[-1] != int(n):
                raise ValueError(f"ref must be an (n,) or (R, n) integer array with n={int(n)}, not {a.dtype} of shape {a.shape}")
            self.ref = np.ascontiguousarray(np.clip(a.reshape(-1, int(n)), -2 ** 31, 2 ** 31 - 1), dtype=np.int32)
        h = C.c_void_p()
        R = self.ref.shape[0]
        _check(lib().pmdi_agreement_create(int(device), int(n_chains), int(K), int(N), int(n), R, _ptr(self.ref) if R else None,
                                           int(trace_cap), C.byref(h)))
        self.h = h
        self.C, self.K, self.N, self.n, self.R, self.device = int(n_chains), int(K), int(N), int(n), R, int(device)
        self.trace_cap = int(trace_cap)
        self.G = self.K * (self.K - 1) // 2
        self.Q = self.G + self.R * self.K

    def add_arrays(self, s):
        """s: CUDA int32 tensor (C, K, n) of 0-based labels, the layout of the resident state."""
        import ctypes as C
        import torch
        t = self._checked_tensor(s, torch.int32, (self.C, self.K, self.n), "add_arrays: s")
        _check(lib().pmdi_agreement_add_arrays(self.h, C.c_void_p(t.data_ptr()), self._stream()))

    def _empty(self):
        C_, Q = self.C, self.Q
        return {"rand_num": np.zeros((C_, Q), dtype=np.int64), "ari_sum": np.zeros((C_, Q)), "ari_sq": np.zeros((C_, Q)),
                "vi_sum": np.zeros((C_, Q), dtype=np.int64), "mi_sum": np.zeros((C_, Q), dtype=np.int64),
                "ari_hist": np.zeros((Q, 256), dtype=np.int64), "trace": np.zeros((self.trace_cap, Q))}

    def arrays(self):
        """Host copies of every array of the accumulator (synchronises the stream; the trace whole, all trace_cap rows); raises
        PmdiError(PMDI_E_DATA) if a label outside 0..N-1 was added since the last reset."""
        out = self._empty()
        _check(lib().pmdi_agreement_get(self.h, *[_ptr(a) if a.size else None for a in out.values()], self._stream()))
        return out

    def last(self):
        """(C, Q, 7) int64: both, jl, px, py, hx, hy, n_q of the latest add (synchronises the stream)."""
        out = np.zeros((self.C, self.Q, 7), dtype=np.int64)
        _check(lib().pmdi_agreement_last(self.h, _ptr(out), self._stream()))
        return out

    def result(self, names=None):
        """The AgreementSummary of everything added so far; its trace holds the rows written (min(T, trace_cap))."""
        a = self.arrays()
        n_q = [self.n] * self.G + [int((self.ref[r] >= 0).sum()) for r in range(self.R) for _ in range(self.K)]
        tr = a.pop("trace")[:min(self.T, self.trace_cap)]
        tr = tr if self.trace_cap else None
        return AgreementSummary(self.T, self.K, n_q, trace=tr, names=names, **a)
