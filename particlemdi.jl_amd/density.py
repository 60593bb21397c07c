"""The log density of the states the chains visit: its trace, the highest-density sampled state, Rao-Blackwellised feature relevance.

DensityAccumulator (include/pmdi_hip.h, pmdi_density_*) evaluates, in every retained state of every chain while it is resident on
the MI355X, the collapsed log likelihood of every dataset given the chain's allocations and feature flags -- the reference's log
marginal as written: the normal-inverse-gamma marginal for Gaussian data, exact for NegBinom, the reference's constant for
Categorical -- the log prior of the allocations given Pi and Phi, and their sum, the log joint (Stan's lp__).  It keeps the three
traces, the maximum-a-posteriori draw of every chain, and per feature the sums of the log Bayes factor "clustered against one
cluster" (src/pmdi.jl:354-367), which is a function of the allocations alone and so exists for runs made without feature
selection.  It ends in a DensityResult, a small host object.  There is no merge: a trace is a sequence in time of one set of
chains; pool the chains of several devices by keeping their DensityResults side by side.
"""
import ctypes as C

import numpy as np

from ._lib import _Accumulator, _check, _ptr, lib
from .summary import PosteriorSummary

Q_ONE = 1 << 20                              # the fixed point of p_sum


class DensityResult:
    """What T adds of C chains say, as plain numpy arrays in the layouts of include/pmdi_hip.h: log_likelihood (T, C, K),
    log_prior (T, C), log_joint (T, C); best_val (C,), best_t (C,) int64 (-1: no state yet), best_s (C, K, n) 0-based labels;
    bf_sum, bf_sq_sum (sumD,) float64, p_sum, bad (sumD,) int64; feature_D: the datasets' feature counts (their sum is sumD).
    Built by DensityAccumulator.result(), or directly from arrays."""

    def __init__(self, log_likelihood, log_prior, log_joint, best_val, best_t, best_s, bf_sum, bf_sq_sum, p_sum, bad, feature_D=None,
                 names=None):
        self.log_likelihood = np.asarray(log_likelihood, dtype=np.float64)
        if self.log_likelihood.ndim != 3:
            raise ValueError(f"log_likelihood must be (T, C, K), not {self.log_likelihood.shape}")
        self.T, self.C, self.K = self.log_likelihood.shape
        self.log_prior = np.asarray(log_prior, dtype=np.float64).reshape(self.T, self.C)
        self.log_joint = np.asarray(log_joint, dtype=np.float64).reshape(self.T, self.C)
        self.best_val = np.asarray(best_val, dtype=np.float64).reshape(self.C)
        self.best_t = np.asarray(best_t, dtype=np.int64).reshape(self.C)
        self.best_s = np.asarray(best_s).reshape(self.C, self.K, -1).astype(np.int32)
        self.n = self.best_s.shape[2]
        self.bf_sum = np.asarray(bf_sum, dtype=np.float64).reshape(-1)
        self.sumD = self.bf_sum.size
        self.bf_sq_sum = np.asarray(bf_sq_sum, dtype=np.float64).reshape(self.sumD)
        self.p_sum = np.asarray(p_sum, dtype=np.int64).reshape(self.sumD)
        self.bad = np.asarray(bad, dtype=np.int64).reshape(self.sumD)
        self.feature_D = [int(d) for d in feature_D] if feature_D is not None else [self.sumD]
        if sum(self.feature_D) != self.sumD:
            raise ValueError(f"feature_D {self.feature_D} does not add up to {self.sumD} features")
        self.names = list(names) if names is not None else [f"K{i}" for i in range(1, self.K + 1)]

    def trace(self):
        """{"log_joint": (T,), "log_prior": (T,), "log_likelihood": (T, K)}: the mean over the chains, draw by draw."""
        return {"log_joint": self.log_joint.mean(axis=1), "log_prior": self.log_prior.mean(axis=1),
                "log_likelihood": self.log_likelihood.mean(axis=1)}

    def rhat(self):
        """The Gelman-Rubin statistic of the log joint and of every dataset's log likelihood over the C chains of T draws
        (PosteriorSummary._rhat on the per-chain mean and sample variance): {"log_joint": float, "log_likelihood": (K,)}."""
        if self.C < 2 or self.T < 2:
            raise ValueError(f"R-hat needs at least 2 chains of at least 2 draws (C={self.C}, T={self.T})")
        lj = self.log_joint[:, :, None]
        r = lambda x: PosteriorSummary._rhat(x.mean(axis=0), x.var(axis=0, ddof=1), self.T)
        return {"log_joint": float(r(lj)[0]), "log_likelihood": r(self.log_likelihood)}

    def best_per_chain(self, device=None):
        """(C, K, n) int32, 0-based: the highest-density state every chain visited, the layout of the draws that
        partition_distances, best_sampled_allocation and minimise_expected_loss(draw_starts=) take.  device=None: a numpy array
        (partition_distances takes it); device=d: a CUDA tensor on cuda:d, what the other two need."""
        if device is None:
            return self.best_s.copy()
        import torch
        return torch.from_numpy(self.best_s.copy()).to(torch.device("cuda", int(device)))

    def best(self):
        """The overall maximum: {"labels": (K, n) 0-based int32, "chain": c, "draw": t, "value": lj}.  The lowest chain wins a
        tie; a chain whose log joint was never above -inf (or always NaN) is no candidate."""
        ok = np.nonzero(self.best_t >= 0)[0]
        if ok.size == 0:
            raise ValueError("DensityResult: no chain has a best state (nothing added, or every log joint was -inf or NaN)")
        c = int(ok[np.argmax(self.best_val[ok])])      # argmax returns the first of equal maxima: the lowest chain
        return {"labels": self.best_s[c].copy(), "chain": c, "draw": int(self.best_t[c]), "value": float(self.best_val[c])}

    def _split(self, v):
        offs = np.concatenate([[0], np.cumsum(self.feature_D)])
        return [v[offs[k]:offs[k + 1]].copy() for k in range(len(self.feature_D))]

    def _good(self):
        if self.T < 1 or self.C < 1:
            raise ValueError("DensityResult: no samples behind the sums")
        return self.T * self.C - self.bad

    def feature_bayes_factor(self, moment="mean"):
        """K arrays (D_k,): the mean over the samples of the log Bayes factor of "feature clustered" against "feature in one
        cluster" given the allocations, or with moment="variance" its sample variance (0 where fewer than two).  Samples whose
        factor was not finite (`bad`) are left out; NaN where none is left."""
        m = self._good().astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = np.where(m > 0, self.bf_sum / np.maximum(m, 1), np.nan)
            if moment == "mean":
                return self._split(mean)
            if moment != "variance":
                raise ValueError('feature_bayes_factor: moment must be "mean" or "variance"')
            var = (self.bf_sq_sum - m * mean * mean) / np.maximum(m - 1, 1)
        return self._split(np.where(m > 1, np.maximum(var, 0.0), 0.0))

    def feature_probs(self):
        """K arrays (D_k,) in the shape get_feature_select_probs returns (data_map(featureSelectProbs=) takes it): the mean of
        pr = 1 - 1 / exp(bf + 1), the probability the reference's coin has (src/pmdi.jl:367), floored at 0 -- the
        Rao-Blackwellised counterpart of the averaged flags."""
        m = self._good()
        return self._split(np.where(m > 0, self.p_sum / (np.maximum(m, 1) * float(Q_ONE)), np.nan))


class DensityAccumulator(_Accumulator):
    """The streaming density accumulator on one MI355X (include/pmdi_hip.h, pmdi_density_*), a child of `sweeper`'s handle.
    After every retained iteration it takes the device-resident allocations, Pi, Phi and feature flags of every chain.
    trace_cap: the adds it can take (the rows of the traces).  Device memory: 8 trace_cap C (K + 2) bytes of traces, C K n bytes
    of best states, a stage buffer of at most PMDI_DENSITY_BUDGET_BYTES (budget= lowers it); keep_last=True keeps the log
    marginals of all chains (8 C sumD N bytes), which is what last() reads.  All calls go to the current torch stream."""
    _prefix = "pmdi_density"
    T = samples = property(_Accumulator._samples, doc="Adds so far = retained draws per chain.")

    def __init__(self, sweeper, trace_cap, keep_last=False, budget=None):
        h = C.c_void_p()
        _check(lib().pmdi_density_create(sweeper.h, int(trace_cap), int(bool(keep_last)), C.byref(h)))
        self.h = h
        self.sw = sweeper      # (the handle outlives its children)
        self.C, self.K, self.N, self.n = sweeper.C, sweeper.K, sweeper.N, sweeper.n
        self.sumD, self.device, self.D = sweeper.sumD, sweeper.device, list(sweeper.D)
        self.trace_cap, self.keep_last, self.G = int(trace_cap), bool(keep_last), sweeper.K * (sweeper.K - 1) // 2
        if budget is not None:
            _check(lib().pmdi_density_set_budget(self.h, int(budget)))

    def add_arrays(self, s, Pi, flags=None, Phi=None):
        """CUDA tensors in the layouts of the resident state: s int32 (C, K, n) 0-based labels, Pi float64 (C, K, N), flags uint8
        (C, sumD) or None = every feature on, Phi float64 (C, max(1, G)) (K = 1: not read, may be None)."""
        import torch
        keep = [self._checked_tensor(s, torch.int32, (self.C, self.K, self.n), "add_arrays: s"),
                self._checked_tensor(Pi, torch.float64, (self.C, self.K, self.N), "add_arrays: Pi")]
        ptrs = [C.c_void_p(t.data_ptr()) for t in keep]
        for t, dtype, shape, what in ((flags, torch.uint8, (self.C, self.sumD), "flags"), (Phi, torch.float64, (self.C, max(1, self.G)), "Phi")):
            if t is not None:
                keep.append(self._checked_tensor(t, dtype, shape, "add_arrays: " + what))
            ptrs.append(None if t is None else C.c_void_p(keep[-1].data_ptr()))
        _check(lib().pmdi_density_add_arrays(self.h, *ptrs, self._stream()))

    def arrays(self):
        """Host copies of the state (synchronises the stream), the traces cut to the T rows written; raises
        PmdiError(PMDI_E_DATA) if a label outside 0..N-1 was added since the last reset."""
        cap, C_, K = self.trace_cap, self.C, self.K
        out = {"log_likelihood": np.zeros((cap, C_, K)), "log_prior": np.zeros((cap, C_)), "log_joint": np.zeros((cap, C_)),
               "best_val": np.zeros(C_), "best_t": np.zeros(C_, dtype=np.int64), "best_s": np.zeros((C_, K, self.n), dtype=np.uint8),
               "bf_sum": np.zeros(self.sumD), "bf_sq_sum": np.zeros(self.sumD), "p_sum": np.zeros(self.sumD, dtype=np.int64),
               "bad": np.zeros(self.sumD, dtype=np.int64)}
        _check(lib().pmdi_density_get(self.h, *[_ptr(a) for a in out.values()], self._stream()))
        T = self.T
        for name in ("log_likelihood", "log_prior", "log_joint"):
            out[name] = out[name][:T].copy()
        return out

    def last(self):
        """The stage outputs of the last add (keep_last=True only; synchronises the device): {"cn", "first": (C, K, N) int32,
        "lm": (C, sumD, N), "bf", "cl": (C, sumD), "q": (C, sumD) int64, "agree": (C, max(1, G)) int64, "logZ": (C,)}."""
        CKN, CD = (self.C, self.K, self.N), (self.C, self.sumD)
        out = {"cn": np.zeros(CKN, dtype=np.int32), "first": np.zeros(CKN, dtype=np.int32), "lm": np.zeros(CD + (self.N,)),
               "bf": np.zeros(CD), "cl": np.zeros(CD), "q": np.zeros(CD, dtype=np.int64),
               "agree": np.zeros((self.C, max(1, self.G)), dtype=np.int64), "logZ": np.zeros(self.C)}
        _check(lib().pmdi_density_last(self.h, *[_ptr(a) for a in out.values()]))
        return out

    def result(self, names=None):
        """The DensityResult of everything added so far."""
        a = self.arrays()
        return DensityResult(*a.values(), feature_D=self.D, names=names)
