"""The HIP kernels' sweep against the closed-form laws of tests/_exact.py: the cases, seeds, sample sizes and bounds of
tests/test_exact_step.py (which asks the same of the oracle on the CPU), on the general kernel as one workgroup per chain, as K
cooperating workgroups (K > 1) and, where the handle supports it, forced onto the settled-chain kernel.  Nothing here is compared
with the oracle."""
import numpy as np
import pytest

import _exact as E
import test_exact_step as S

pytestmark = pytest.mark.gpu

GENERAL = {"settled": 0, "ksplit": 0}
KSPLIT = {"settled": 0, "ksplit": 1}
SETTLED = {"settled": 2, "sticky": 0, "ksplit": 0}


def kernels(case):
    return [("general", GENERAL)] + ([("k-split", KSPLIT), ("settled", SETTLED)] if case.K > 1 else [])


def run_gpu(pkg, case, name, tuning, chains, seed=S.SEED):
    """`chains` chains (seeds seed, seed + 1, ...) of the same case on one handle -> list of per-chain results, or None when the
    handle does not put this shape on the settled-chain kernel."""
    sw = pkg.Sweeper(case.data, case.kinds, case.N, case.P, n_chains=chains, seed=seed, tuning=tuning)
    try:
        if name == "settled" and not sw.settled:
            return None
        rep = lambda a: np.repeat(np.asarray(a)[None], chains, axis=0)
        r = sw.sweep(case.it, rep(case.s), rep(case.order), case.n1, rep(case.Pi), rep(case.Phi),
                     None if case.flags_flat is None else rep(case.flags_flat), trace=True)
        by = sw.swept_by()
        if name == "settled":
            assert np.isin(by, (1, 2)).all(), by
        else:
            assert (by == 0).all(), by
        return [{"s": r["s"][c], "p_star": int(r["p_star"][c]), "logweight": r["logweight"][c], "trace": r["trace"][c],
                 "state": sw.export_state(c)} for c in range(chains)]
    finally:
        sw.close()


@pytest.mark.parametrize("c", E.weight_cases(), ids=E.case_id)
def test_logweights_and_reference_particle(pkg, c):
    case = E.StepCase(*c)
    law = case.law()
    for name, tuning in kernels(case):
        res = run_gpu(pkg, case, name, tuning, 2)
        if res is None:
            continue
        for ch, r in enumerate(res):
            labels = E.labels_from_export(r["state"], law.prefix_count)
            assert (labels[0] == case.s[case.row]).all(), "particle 0 carries s_in at the swept observation"
            assert (r["s"][case.row] == labels[r["p_star"] - 1]).all() and (np.delete(r["s"], case.row, 0) == np.delete(case.s, case.row, 0)).all()
            S.check_weights(case, law, r, labels, S.ULPS, f"{name} chain {ch}")


@pytest.mark.parametrize("c", E.draw_cases(), ids=E.case_id)
def test_draws_follow_the_closed_form_and_are_independent(pkg, c):
    case = E.StepCase(*c)
    law = case.law()
    for name, tuning in kernels(case):
        res = run_gpu(pkg, case, name, tuning, S.n_chains(case.P))
        if res is None:
            continue
        lab = np.stack([E.labels_from_export(r["state"], law.prefix_count) for r in res])
        for what, obs, exp in S.draw_statistics(case, law, lab):
            p, bins = E.chi2_pvalue(obs, exp)
            print(f"{name} {what}: p = {p:.3g} over {bins} bins, {int(obs.sum())} samples")
            assert bins >= 2 and p >= E.P_FLOOR, (name, what, p)


@pytest.mark.parametrize("c", S.RESAMPLING_CASES, ids=E.case_id)
def test_resampling_is_systematic_and_keeps_particle_0(pkg, c):
    """As tests/test_exact_step.py's test of the same name: the labels before the resampling come from the same seeds with a small
    Phi, the resampled export must be an outcome of systematic resampling of their exact weights with particle 0 kept."""
    quiet, loud = E.StepCase(*c), E.StepCase(*c, phi=40.0)
    law = loud.law()
    for name, tuning in kernels(loud):
        qa, lo = run_gpu(pkg, quiet, name, tuning, 2), run_gpu(pkg, loud, name, tuning, 2)
        if qa is None:
            continue
        for rq, r in zip(qa, lo):
            S.check_resampled(loud, law, E.labels_from_export(rq["state"], law.prefix_count), r)


def test_stationary_law_of_the_sweep_with_per_step_class_ids(pkg):
    """tests/test_exact_chain.py on the device: 2 048 independent chains of the n = 6, N = 3 problem (q1_mode = 1, which only the
    general kernel runs), 40 sweeps each from the all-ones start; the chains' final allocations are 2 048 independent draws from the
    stationary law, compared with the enumerated posterior."""
    import test_exact_chain as T
    C_, P = 2048, 64
    pt = T.target()
    sw = pkg.Sweeper([T.X], ["categorical"], T.N_LAB, P, n_chains=C_, seed=S.SEED, q1_mode=1)
    rng = np.random.default_rng(3)
    s = np.ones((C_, T.N_OBS, 1), dtype=np.int64)
    Pi = np.repeat(T.PI[None], C_, axis=0)
    for it in range(1, 41):
        order = np.stack([rng.permutation(T.N_OBS) + 1 for _ in range(C_)])
        s = sw.sweep(it, s, order, 1, Pi, np.zeros((C_, 1)))["s"]
    assert (sw.swept_by() == 0).all()
    sw.close()
    counts = np.bincount(T.state_index(s[:, :, 0]), minlength=len(T.STATES))
    p, bins = E.chi2_pvalue(counts, pt * counts.sum())
    print(f"{C_} chains: p = {p:.3g} over {bins} bins")
    assert bins >= 20 and p >= E.P_FLOOR
