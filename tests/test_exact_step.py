"""The oracle's sweep against closed-form laws (tests/_exact.py: 50-digit arithmetic, written from the reference's cluster definitions,
sharing no code, table or random stream with oracle/ or the kernels).

With n1 = n the first n - 1 observations of order_obs are a prefix of known labels and only the last one is swept
(src/pmdi.jl:192-209): every particle holds the same clusters, so each free particle's label is an independent draw from
f_k = Pi[:, k] * pred_k / sum, and its log-weight is an exact number given its labels.  tests/test_gpu_exact_step.py asks the same of
the HIP kernels, with the same cases, seeds and sample sizes.

Every statistical assertion uses fixed seeds and the threshold p >= 1e-6 (107 such assertions here: a correct sweep fails one with
probability about 1e-4, and never again once these seeds have been seen to pass).
"""
import numpy as np
import pytest

import _exact as E

# Units in the last place between a log-weight and its exact value.  Categorical: 4, as one log of a ratio per feature allows; the
# oracle stays within it on every case here.  NegBinom: the oracle alone exceeds 4 on the CPU -- its log-predictive is six lgamma
# values per feature, of size up to a few hundred, whose differences cancel -- by up to 59 units over the 84 cases below (seeds SEED,
# SEED + 1; measured on the oracle, never on a kernel), so the bound is twice that measurement.
MEASURED_ORACLE_NEGBINOM_ULPS = 59
ULPS = 2 * MEASURED_ORACLE_NEGBINOM_ULPS
SEED = 4100
SAMPLES = 60000          # free-particle draws pooled per case (chains = ceil(SAMPLES / P), at least 16)


def n_chains(P):
    return max(16, -(-SAMPLES // P))


def run_oracle(O, case, seed, trace=True):
    o = O.Oracle(case.data, case.kinds, case.N, case.P, seed=seed)
    r = o.sweep(case.it, case.s, case.order, case.n1, case.Pi, case.Phi, flags=case.flags, trace=trace)
    r["state"] = o.export()
    o.close()
    return r


def check_weights(case, law, r, labels, ulps, where=""):
    """Every particle's exported log-weight against the closed form for its labels; returns the largest error in units of the
    tolerance's discrete part (for the docstring's measurement)."""
    assert r["trace"][-1, 1] == 0, "the case is built not to resample after the swept observation"
    match = np.stack([labels[:, a] == labels[:, b] for a, b in E.phi_pairs(case.K)], axis=1) if case.K > 1 else np.zeros((case.P, 0), bool)
    code = (match * (1 << np.arange(match.shape[1]))).sum(axis=1)
    worst = 0.0
    for c in np.unique(code):
        p0 = int(np.nonzero(code == c)[0][0])
        exact = float(law.logweight(labels[p0], case.lw_init))
        err = np.abs(r["logweight"][code == c] - exact).max()
        tol = case.tolerance(exact, ulps)
        worst = max(worst, err / float(np.spacing(abs(exact))))
        print(f"{where} pairs-matched code {c}: exact {exact!r} max |error| {err:.3e} tolerance {tol:.3e}")
        assert err <= tol, (where, c, exact, err, tol)
    return worst


@pytest.mark.parametrize("c", E.weight_cases(), ids=E.case_id)
def test_logweights_and_reference_particle(O, c):
    case = E.StepCase(*c)
    law = case.law()
    for seed in (SEED, SEED + 1):
        r = run_oracle(O, case, seed)
        labels = E.labels_from_export(r["state"], law.prefix_count)
        assert (labels[0] == case.s[case.row]).all(), "particle 0 carries s_in at the swept observation"
        assert (r["s"][case.row] == labels[r["p_star"] - 1]).all() and (np.delete(r["s"], case.row, 0) == np.delete(case.s, case.row, 0)).all()
        check_weights(case, law, r, labels, ULPS, f"seed {seed}")


def pooled_labels(O, case, law):
    return np.stack([E.labels_from_export(run_oracle(O, case, SEED + ch)["state"], law.prefix_count) for ch in range(n_chains(case.P))])


def draw_statistics(case, law, lab):
    """lab: (chains, P, K) labels -> [(name, observed counts, expected counts)] for the draws (per dataset), the joint law of dataset
    pairs, neighbouring particles (p, p + 1) and the same particle in neighbouring chains."""
    N, K = case.N, case.K
    free = lab[:, 1:, :] - 1                                           # particle 0 is the reference trajectory
    f = [law.f_float(k) for k in range(K)]
    out = []
    for k in range(K):
        out.append((f"draws k={k}", np.bincount(free[:, :, k].ravel(), minlength=N), f[k] * free[:, :, k].size))
    for a, b in E.phi_pairs(K):
        joint = np.bincount((free[:, :, a] * N + free[:, :, b]).ravel(), minlength=N * N)
        out.append((f"joint k={a},{b}", joint, np.outer(f[a], f[b]).ravel() * free[:, :, a].size))
    m = (free.shape[1] // 2) * 2
    x, y = free[:, 0:m:2, 0], free[:, 1:m:2, 0]
    out.append(("particles p,p+1", np.bincount((x * N + y).ravel(), minlength=N * N), np.outer(f[0], f[0]).ravel() * x.size))
    c2 = (free.shape[0] // 2) * 2
    x, y = free[0:c2:2, :, 0], free[1:c2:2, :, 0]
    out.append(("chains c,c+1", np.bincount((x * N + y).ravel(), minlength=N * N), np.outer(f[0], f[0]).ravel() * x.size))
    return out


@pytest.mark.parametrize("c", E.draw_cases(), ids=E.case_id)
def test_draws_follow_the_closed_form_and_are_independent(O, c):
    case = E.StepCase(*c)
    law = case.law()
    lab = pooled_labels(O, case, law)
    stats = draw_statistics(case, law, lab)
    for name, obs, exp in stats:
        p, bins = E.chi2_pvalue(obs, exp)
        print(f"{name}: p = {p:.3g} over {bins} bins, {int(obs.sum())} samples")
        assert bins >= 2, f"{name}: the case leaves nothing to test"
        assert p >= E.P_FLOOR, (name, p)
    # sensitivity: the same counts against the law with two Pi entries swapped (the two labels dataset 0 draws most) must be rejected
    f0 = law.f_float(0)
    a, b = np.argsort(f0)[-2:]
    Pi = case.Pi.copy()
    Pi[[a, b], 0] = Pi[[b, a], 0]
    wrong = case.law(Pi).f_float(0)
    name, obs, _ = stats[0]
    p, _ = E.chi2_pvalue(obs, wrong * obs.sum())
    print(f"sensitivity: Pi[{a}] <-> Pi[{b}] in the expected law: p = {p:.3g}")
    assert p < E.P_FLOOR, "the sample is too small to see a one-slot error in Pi"
    # ... and a CDF read one slot off (label c drawn where c + 1 is due)
    p, _ = E.chi2_pvalue(obs, np.roll(f0, 1) * obs.sum())
    assert p < E.P_FLOOR


RESAMPLING_CASES = [(("gaussian", "categorical"), 10, 1024, 0), (("categorical", "negbinom"), 2, 256, 0),
                    (("gaussian", "categorical", "negbinom"), 10, 2048, 1), (("gaussian", "gaussian", "gaussian"), 64, 4096, 0)]


def check_resampled(loud, law, before, r, seed=0):
    """before: (P, K) labels of every particle before the resampling; r: the resampled sweep's result with its exported state."""
    assert r["trace"][-1, 1] == 1 and r["trace"][-1, 0] <= 0.5 * loud.P, "the case is built to resample"
    assert (r["logweight"] == 1.0).all()                                        # src/pmdi.jl:319
    after = E.labels_from_export(r["state"], law.prefix_count)
    lw = np.array([float(law.logweight(l, loud.lw_init)) for l in before])
    w = np.exp(lw - lw.max())
    key = lambda lab: (lab * (loud.N + 1) ** np.arange(loud.K)).sum(axis=1)
    assert (after[0] == loud.s[loud.row]).all(), "particle 0 survives the resampling"
    assert E.systematic_family_contains(w / w.sum(), key(before), key(after))
    # sensitivity: multinomial resampling of the same weights is not a member
    fake = np.sort(np.random.default_rng(seed).choice(loud.P, size=loud.P, p=w / w.sum()))
    fake[0] = 0
    assert not E.systematic_family_contains(w / w.sum(), key(before), key(before)[fake])


@pytest.mark.parametrize("c", RESAMPLING_CASES, ids=E.case_id)
def test_resampling_is_systematic_and_keeps_particle_0(O, c):
    """Phi = 40 makes the weights after the swept observation so uneven that the ESS falls below P / 2 and the particles are resampled
    (src/pmdi.jl:317-341 runs after the last swept observation too, and the exported state is the resampled one).  The draws do not
    depend on Phi, so the same seed with a small Phi shows every particle's labels BEFORE the resampling; their exact weights span the
    family of outcomes the reference's systematic resampling can produce (each ancestor floor(P w) or ceil(P w) times, in order, one
    slot given to particle 0), and the resampled state must be a member.  (One swept observation, not two: a second one would draw
    again on top of the resampled particles and the export could no longer tell which label belongs to which observation.)"""
    quiet = E.StepCase(*c)
    loud = E.StepCase(*c, phi=40.0)
    assert all((a == b).all() for a, b in zip(quiet.data, loud.data)) and (quiet.s == loud.s).all() and (quiet.Pi == loud.Pi).all()
    law = loud.law()
    for seed in (SEED, SEED + 1):
        before = E.labels_from_export(run_oracle(O, quiet, seed)["state"], law.prefix_count)
        check_resampled(loud, law, before, run_oracle(O, loud, seed), seed)
