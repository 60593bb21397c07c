"""Leave-one-out fit of the TRAINING observations: which rows does the fitted mixture explain badly, and which model fits better?

LooAccumulator (include/pmdi_hip.h, pmdi_loo_*) evaluates, in every retained state of every chain while it is resident on the
MI355X, the Gibbs full conditional of every training row's allocation with the row taken out of its own cluster, and sums the log
conditional predictive density, the exact harmonic-mean pair (E, S) behind the conditional predictive ordinate CPO_i = p(x_i | the
other data), and the fixed-point mass on the row's own label and on an empty label.  It ends in a LooCounts, a small host object:
log CPO per row and dataset, the log pseudo-marginal likelihood (LPML, to compare kinds, N, or sets of datasets on the same rows),
a stability score and an outlier score.  With coupled=True the weights carry Phi against the labels the other datasets give the row.
"""
import ctypes as C
import math

import numpy as np

from ._lib import _Accumulator, _check, _ptr, lib

Q_ONE = 1 << 20                              # the fixed point of p_own and p_new
E_EMPTY = -9187201950435737472               # PMDI_LOO_E_EMPTY: a pair nothing was added to
_SUMS = (("own_sum", np.int64), ("new_sum", np.int64), ("zero", np.int64), ("lcp_sum", np.float64), ("lcp_sq_sum", np.float64),
         ("E", np.int64), ("S", np.int64))      # the order of pmdi_loo_get's and pmdi_loo_merge's arguments


BINS, BIN_BITS, MANT_BITS = 3, 32, 52         # the pair keeps the three highest bins of 32 binades; mant is an integer times 2^-52
_U64 = (1 << 64) - 1


def pair_add(E, S, e, mant):
    """One term mant 2^e into the pair: the rule of include/pmdi_hip.h, step 7, on Python integers.  E: the highest bin index or
    E_EMPTY; S: the BINS exact bin sums (Python ints), highest bin first.  Returns the new (E, S)."""
    m = int(mant * 4503599627370496.0) if 0.0 <= mant < 4.0 else 0
    return bin_add(E, S, e >> 5, m << (e & 31))


def bin_add(E, S, b, v):
    """The integer v into absolute bin b."""
    S = list(S)
    if E == E_EMPTY or b > E:
        d = BINS if E == E_EMPTY else b - E
        S = ([0] * min(d, BINS) + S)[:BINS]
        E = b
    if E - b < BINS:
        S[E - b] += v
    return E, S


def pair_merge(E, S, E_b, S_b):
    """Another pair into this one, bin by bin."""
    if E_b == E_EMPTY:
        return E, list(S)
    for j in range(BINS):
        E, S = bin_add(E, S, E_b - j, S_b[j])
    return E, S


def pack_bins(S):
    """BINS Python ints -> 2 BINS int64 words (high, low) per bin, as the device holds them."""
    words = []
    for v in S:
        words += [(v >> 64) & _U64, v & _U64]
    return np.array(words, dtype=np.uint64).view(np.int64)


def unpack_bins(words):
    w = [int(x) for x in np.asarray(words, dtype=np.int64).view(np.uint64)]
    return [(w[2 * j] << 64) | w[2 * j + 1] for j in range(BINS)]


class LooCounts:
    """What T adds of C chains say about the n training rows of K datasets, as plain numpy (K, n) arrays in the layouts of
    include/pmdi_hip.h: own_sum, new_sum, zero (int64), lcp_sum, lcp_sq_sum (float64) and the exact pair E (K, n) int64, S (K, n, 6) int64 (the
    high and low words of its three highest exponent bins).
    Built by LooAccumulator.result(), or directly from arrays."""

    def __init__(self, T, C, own_sum, new_sum, zero, lcp_sum, lcp_sq_sum, E, S, names=None):
        self.T, self.C = int(T), int(C)
        self.own_sum = np.asarray(own_sum, dtype=np.int64)
        if self.own_sum.ndim != 2:
            raise ValueError(f"own_sum must be (K, n), not {self.own_sum.shape}")
        self.K, self.n = self.own_sum.shape
        shape = (self.K, self.n)
        self.new_sum = np.asarray(new_sum, dtype=np.int64).reshape(shape)
        self.zero = np.asarray(zero, dtype=np.int64).reshape(shape)
        self.lcp_sum = np.asarray(lcp_sum, dtype=np.float64).reshape(shape)
        self.lcp_sq_sum = np.asarray(lcp_sq_sum, dtype=np.float64).reshape(shape)
        self.E = np.asarray(E, dtype=np.int64).reshape(shape)
        self.S = np.asarray(S, dtype=np.int64).reshape(shape + (2 * BINS,))
        self.names = list(names) if names is not None else [f"K{i}" for i in range(1, self.K + 1)]

    def _samples(self):
        if self.T < 1 or self.C < 1:
            raise ValueError("LooCounts: no samples behind the counts")
        return self.T * self.C

    def _finite(self):
        """(K, n): the samples whose conditional density was finite and positive."""
        return self._samples() - self.zero

    def log_cpo(self):
        """(K, n): log CPO = -(log sum exp(-ell) - log(T C - zero)), the sum read exactly from the bins; -inf where a sample gave
        the row no density at all (zero > 0)."""
        m = self._finite()
        out = np.full((self.K, self.n), -np.inf)
        for k, i in zip(*np.nonzero((self.zero == 0) & (self.E != E_EMPTY) & (m > 0))):
            bins = unpack_bins(self.S[k, i])
            total = sum(v << (BIN_BITS * (BINS - 1 - j)) for j, v in enumerate(bins))      # in units of 2^(32 (E - 2) - 52)
            if total > 0:
                scale = BIN_BITS * (int(self.E[k, i]) - (BINS - 1)) - MANT_BITS
                out[k, i] = -(scale * math.log(2.0) + math.log(total) - math.log(int(m[k, i])))
        return out

    def lpml(self, total=False):
        """(K,): the log pseudo-marginal likelihood of every dataset, the sum of log CPO over its rows; total=True: their sum."""
        v = self.log_cpo().sum(axis=1)
        return float(v.sum()) if total else v

    def log_conditional(self, moment="mean"):
        """(K, n): the mean over the finite samples of the log conditional predictive density of the row, or with
        moment="variance" its variance over them (0 where fewer than two)."""
        m = np.maximum(self._finite(), 1)
        mean = self.lcp_sum / m
        if moment == "mean":
            return mean
        if moment != "variance":
            raise ValueError('log_conditional: moment must be "mean" or "variance"')
        var = (self.lcp_sq_sum - m * mean * mean) / np.maximum(m - 1, 1)
        return np.where(m > 1, np.maximum(var, 0.0), 0.0)

    def own_label(self):
        """(K, n): the mean full-conditional probability of the label the chain holds for the row -- a Rao-Blackwellised
        stability score."""
        return self.own_sum / float(self._samples() * Q_ONE)

    def new_cluster(self):
        """(K, n): the mean full-conditional mass on an empty label -- the outlier score, the training rows' counterpart of
        PredictiveCounts.new_cluster."""
        return self.new_sum / float(self._samples() * Q_ONE)

    def outliers(self, level=0.05, k=None):
        """The worst-explained rows: the indices of the ceil(level n) rows of lowest log CPO, worst first -- of dataset k, or by
        the sum over the datasets when k is None."""
        if not 0.0 < level <= 1.0:
            raise ValueError("outliers: level must be in (0, 1]")
        score = self.log_cpo().sum(axis=0) if k is None else self.log_cpo()[k]
        return np.argsort(score, kind="stable")[:int(math.ceil(level * self.n))]


class LooAccumulator(_Accumulator):
    """The streaming leave-one-out accumulator on one MI355X (include/pmdi_hip.h, pmdi_loo_*), a child of `sweeper`'s handle.
    After every retained iteration it takes the device-resident allocations, Pi, feature flags and (coupled=True, K >= 2) Phi of
    every chain.  Device memory: the stage buffers of a batch of chains (at most PMDI_LOO_BUDGET_BYTES; budget= lowers it) and
    96 K n bytes of sums; keep_last=True keeps the log predictives of all chains (8 C K n N bytes), which is what last() reads.
    All calls go to the current torch stream of the device."""
    _prefix = "pmdi_loo"
    T = samples = property(_Accumulator._samples, doc="Adds so far = retained draws per chain.")

    def __init__(self, sweeper, coupled=False, keep_last=False, budget=None):
        h = C.c_void_p()
        _check(lib().pmdi_loo_create(sweeper.h, int(bool(coupled)), int(bool(keep_last)), C.byref(h)))
        self.h = h
        self.sw = sweeper      # (the handle outlives its children)
        self.C, self.K, self.N, self.n = sweeper.C, sweeper.K, sweeper.N, sweeper.n
        self.sumD, self.device = sweeper.sumD, sweeper.device
        self.coupled, self.keep_last, self.G = bool(coupled), bool(keep_last), sweeper.K * (sweeper.K - 1) // 2
        if budget is not None:
            _check(lib().pmdi_loo_set_budget(self.h, int(budget)))

    def add_arrays(self, s, Pi, flags=None, Phi=None):
        """CUDA tensors in the layouts of the resident state: s int32 (C, K, n) 0-based labels, Pi float64 (C, K, N), flags uint8
        (C, sumD) or None = every feature on, Phi float64 (C, G) for a coupled accumulator and None for an uncoupled one."""
        import torch
        keep = [self._checked_tensor(s, torch.int32, (self.C, self.K, self.n), "add_arrays: s"),
                self._checked_tensor(Pi, torch.float64, (self.C, self.K, self.N), "add_arrays: Pi")]
        ptrs = [C.c_void_p(t.data_ptr()) for t in keep]
        for t, dtype, shape, what in ((flags, torch.uint8, (self.C, self.sumD), "flags"), (Phi, torch.float64, (self.C, self.G), "Phi")):
            if t is not None:
                keep.append(self._checked_tensor(t, dtype, shape, "add_arrays: " + what))
            ptrs.append(None if t is None else C.c_void_p(keep[-1].data_ptr()))
        _check(lib().pmdi_loo_add_arrays(self.h, *ptrs, self._stream()))

    def arrays(self):
        """Host copies of the seven sums (synchronises the stream); raises PmdiError(PMDI_E_DATA) if a label outside 0..N-1 was
        added since the last reset."""
        out = {name: np.zeros((self.K, self.n) + ((2 * BINS,) if name == "S" else ()), dtype=dtype) for name, dtype in _SUMS}
        _check(lib().pmdi_loo_get(self.h, *[_ptr(a) for a in out.values()], self._stream()))
        return out

    def last(self):
        """The stage outputs of the last add (keep_last=True only; synchronises the device): {"lp": (C, K, n, N) float64, "ell":
        (C, K, n) float64, "p_own", "p_new": (C, K, n) int32 (p_own = -1: a degenerate row), "e": (C, K, n) int64, "mant": (C, K, n)}."""
        rows = (self.C, self.K, self.n)
        out = {"lp": np.zeros(rows + (self.N,)), "ell": np.zeros(rows), "p_own": np.zeros(rows, dtype=np.int32),
               "p_new": np.zeros(rows, dtype=np.int32), "e": np.zeros(rows, dtype=np.int64), "mant": np.zeros(rows)}
        _check(lib().pmdi_loo_last(self.h, *[_ptr(a) for a in out.values()]))
        return out

    def merge(self, other):
        """Adds what another accumulator of the same shape on the same device has seen (or a LooCounts of it): the integer sums
        are added, the Float64 sums are ours + theirs, their pair goes into ours bin by bin (exact), T += theirs."""
        import torch
        lc = other.result() if isinstance(other, LooAccumulator) else other
        if (lc.K, lc.n, lc.C) != (self.K, self.n, self.C):
            raise ValueError(f"merge needs the same K, n, C: {(self.K, self.n, self.C)} vs {(lc.K, lc.n, lc.C)}")
        dev = torch.device("cuda", self.device)
        t = [torch.from_numpy(np.ascontiguousarray(getattr(lc, name))).to(dev) for name, _ in _SUMS]
        _check(lib().pmdi_loo_merge(self.h, *[C.c_void_p(x.data_ptr()) for x in t], int(lc.T), self._stream()))
        torch.cuda.current_stream(dev).synchronize()      # the uploads may go once the kernel has read them

    def result(self, names=None):
        """The LooCounts of everything added so far."""
        a = self.arrays()
        return LooCounts(self.T, self.C, *[a[name] for name, _ in _SUMS], names=names)
