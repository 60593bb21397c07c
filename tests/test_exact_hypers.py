"""The oracle's hyper-parameter updates against closed-form laws (tests/_exact_hypers.py: written from src/update_hypers.jl,
src/misc.jl:61-96 and src/pmdi.jl:59-96,172-185, sharing no code, table or random stream with oracle/, tests/_np_hypers.py or the
kernels).  Nothing here is compared with the oracle's own arithmetic: C = 4096 independent chains (seeds SEED + c) leave one common,
hand-set state through one step, every draw of every chain becomes a probability-integral transform conditioned on what that chain
drew before it, and the transforms are tested for uniformity and for independence.  tests/test_gpu_exact_hypers.py asks the same of
the HIP kernels (gibbs_init_kernel, hypers_kernel, align_kernel) with the same cases, seeds, chain counts, bins and bounds.

Every statistical assertion uses fixed seeds and the threshold p >= E.P_FLOOR = 1e-6.  There are 175 of them here (one step: 21 + 8 +
14 + 15 over the four cases; independence: 19; initial state: 17 + 11 + 67; align_labels!: 3), so a correct implementation fails
one with probability about 1.8e-4, and never again once these seeds have been seen to pass.  (The five assertions of
test_a_wrong_law_is_rejected ask for p < P_FLOOR and are not among them.)  C, the bin counts and the cases are fixed here; the
p-values measured on the oracle on the CPU are quoted beside the tests.
"""
import numpy as np
import pytest

import _exact as E
import _exact_hypers as H

SEED = 100
C = 4096                 # chains per case
BINS = 32                # equal-width bins of a transform
RTOL_Z = 1e-10           # update_Z against the brute-force sum

# n = 12, N = 3, K = 3: label 3 empty in datasets 1 and 2 (shape M / N = 0.4 and 0.67 < 1: the boost) beside occupied labels,
# gamma != gamma0, uneven Phi, v away from n / Z.
S_MAIN = np.array([[1, 1, 1], [1, 1, 2], [1, 2, 3], [1, 2, 3], [1, 1, 1], [2, 2, 2], [2, 2, 3], [2, 1, 1], [2, 2, 2], [1, 2, 3],
                   [2, 2, 3], [1, 1, 1]])
G_MAIN = np.array([[.7, .2, 1.1], [.4, .9, .3], [.05, .6, .8]])
G0_MAIN = np.array([[.5, .3, .2], [.1, .6, .9], [.8, .2, .4]])
_rng = np.random.default_rng(300)
_z300 = _rng.integers(1, 4, 300)
CASES = {
    "main": H.State(S_MAIN, G_MAIN, G0_MAIN, M=(1.2, 2.0, 0.6), Phi=(0.8, 2.5, 0.3), v=0.9, order=[5, 12, 1, 8, 3, 10, 7, 2, 11, 6, 9, 4]),
    "K1": H.State(S_MAIN[:, 2:], G_MAIN[:, 2:], G0_MAIN[:, 2:], M=(0.6,), Phi=(0.0,), v=7.0),
    "K2": H.State(S_MAIN[:, [0, 2]], G_MAIN[:, :2], G0_MAIN[:, 1:], M=(2.5, 0.9), Phi=(1.4,), v=3.0),
    # n = 300: the shuffle works through its positions in chunks of 256
    "n300": H.State(np.stack([_z300, np.where(_rng.random(300) < 0.5, _z300, _rng.integers(1, 3, 300))], axis=1),
                    [[.5, .2], [.3, .7], [.2, .1]], [[.4, .3], [.2, .5], [.4, .2]], M=(1.5, 0.8), Phi=(0.6,), v=250.0,
                    order=_rng.permutation(300) + 1),
}
SHUFFLE_GROUP = {"main": 1, "K1": 1, "K2": 1, "n300": 25}


def run_oracle(O, st, chains=C, seed=SEED, it=1):
    """One hyper-parameter step (src/pmdi.jl:172-185, iteration `it`) of `chains` chains from st -> their states afterwards."""
    out = {"M": [], "gamma": [], "Phi": [], "v": [], "Z": [], "order": [], "s": []}
    for c in range(chains):
        hy = O.Hypers(st.n, st.N, st.K, seed=seed + c)
        hy.s[:] = st.s
        hy.order[:] = st.order
        hy.gamma0, hy.gamma, hy.M, hy.Phi, hy.v = st.gamma0, st.gamma, st.M, st.Phi, st.v
        hy.step(it)
        for key in ("M", "gamma", "Phi", "v", "Z"):
            out[key].append(getattr(hy, key))
        out["order"].append(np.array(hy.order))
        out["s"].append(np.array(hy.s))
        hy.close()
    return {key: np.array(val) for key, val in out.items()}


def run_oracle_init(O, n, N, K, chains=C, seed=SEED):
    out = {"M": [], "gamma": [], "gamma0": [], "Phi": [], "v": [], "Z": [], "order": [], "s": []}
    for c in range(chains):
        hy = O.Hypers(n, N, K, seed=seed + c)
        for key in ("M", "gamma", "gamma0", "Phi", "v", "Z"):
            out[key].append(getattr(hy, key))
        out["order"].append(np.array(hy.order))
        out["s"].append(np.array(hy.s))
        hy.close()
    return {key: np.array(val) for key, val in out.items()}


def run_oracle_align(O, st, chains=C, seed=SEED):
    out = {"gamma": [], "s": []}
    for c in range(chains):
        hy = O.Hypers(st.n, st.N, st.K, seed=seed + c)
        hy.s[:] = st.s
        hy.gamma, hy.Phi = st.gamma, st.Phi
        hy.align_labels(1)
        out["gamma"].append(hy.gamma)
        out["s"].append(np.array(hy.s))
        hy.close()
    return {key: np.array(val) for key, val in out.items()}


def uniformity(U, floors, where=""):
    """-> {site: p} of every site's transforms on BINS equal-width bins."""
    ps = {}
    for name, u in U.items():
        obs, exp = H.uniform_counts(u, BINS, floors.get(name, 0.0))
        ps[name], bins = E.chi2_pvalue(obs, exp)
        print(f"{where} {name}: p = {ps[name]:.3g} over {bins} bins")
        assert bins >= BINS // 2, f"{name}: too few bins are left to test"
    return ps


def m_statistics(st, out, prior_scale=0.25):
    """-> [(name, p)]: per dataset, the share of chains whose M moved (binomial) and the moved values (chi-square on fixed bins)."""
    res = []
    for k in range(st.K):
        law = H.MLaw(st.M[k], st.gamma[:, k], prior_scale)
        moved = out["M"][:, k] != st.M[k]
        res.append((f"M[{k}] moved {int(moved.sum())} of {len(moved)}, law {law.p_move:.4f}",
                    H.binomial_pvalue(moved.sum(), len(moved), law.p_move)))
        obs, exp = law.moved_counts(out["M"][moved, k])
        p, bins = E.chi2_pvalue(obs, exp)
        assert bins >= 8
        res.append((f"M[{k}] moved values over {bins} bins", p))
    return res


def check_step(st, out, group, where=""):
    """Every law of one step; returns the number of statistical assertions made."""
    assert (out["s"] == st.s).all(), "the hyper-parameter step does not touch the allocations"
    U, floors, Z = H.step_transforms(st, out)
    assert np.allclose(out["Z"], Z, rtol=RTOL_Z, atol=0), "update_Z: not the brute-force sum over the N^K table"
    count = 0
    for name, p in uniformity(U, floors, where).items():
        assert p >= E.P_FLOOR, (where, name, p)
        count += 1
    for name, p in m_statistics(st, out):
        print(f"{where} {name}: p = {p:.3g}")
        assert p >= E.P_FLOOR, (where, name, p)
        count += 1
    for name, obs, exp in H.shuffle_tables(out["order"], group):
        p, bins = E.chi2_pvalue(obs, exp)
        print(f"{where} shuffle, {name}: p = {p:.3g} over {bins} bins")
        assert bins >= 100 and p >= E.P_FLOOR, (where, name, p)
        count += 1
    return count


# p-values measured on the oracle on the CPU, C = 4096, BINS = 32, seeds 100...4195 (smallest ... largest of each kind):
#   main   13 gamma / Phi / v sites 0.0084 ... 0.76; 6 of M 0.21 ... 1.0; 2 of the shuffle 0.74, 0.79
#   K1      4 sites 0.44 ... 0.78;  2 of M 0.23, 0.43;        shuffle 0.74, 0.79
#   K2      8 sites 0.0049 ... 0.87; 4 of M 0.22 ... 0.60;    shuffle 0.74, 0.79
#   n300    8 sites 0.0089 ... 0.83; 4 of M 0.35 ... 0.77;    3 of the shuffle 0.37 ... 0.50
# (the smallest is gamma[1,1] every time: that site's shape is large in all three cases, and a large-shape draw is almost a
# function of its normal, which the seeds share.)
@pytest.mark.parametrize("name", list(CASES))
def test_one_step_follows_the_closed_form_laws(O, name):
    st = CASES[name]
    print("statistical assertions:", check_step(st, run_oracle(O, st), SHUFFLE_GROUP[name], name))


def independence_statistics(st, out1, out2):
    """4 x 4 contingency tables of transform pairs against the product law.  out1, out2: iterations 1 and 2 from the same state."""
    U1, _, _ = H.step_transforms(st, out1)
    U2, _, _ = H.step_transforms(st, out2)
    duos = [("two labels of one dataset", U1["gamma[0,0]"], U1["gamma[1,0]"]),
            ("two labels of one dataset (boost, no boost)", U1["gamma[2,1]"], U1["gamma[1,1]"]),
            ("one label in two datasets", U1["gamma[0,0]"], U1["gamma[0,1]"]),
            ("one label in two datasets (both boost)", U1["gamma[2,0]"], U1["gamma[2,1]"]),
            ("Phi of consecutive pairs 0,1", U1["Phi[0]"], U1["Phi[1]"]),
            ("Phi of consecutive pairs 1,2", U1["Phi[1]"], U1["Phi[2]"]),
            ("Phi against v", U1["Phi[2]"], U1["v"]),
            # sites whose draw keys would coincide if two sites shared one random stream: (label 0, dataset i), (pair i), v
            ("gamma[0,0] against Phi[0]", U1["gamma[0,0]"], U1["Phi[0]"]),
            ("gamma[0,1] against Phi[1]", U1["gamma[0,1]"], U1["Phi[1]"]),
            ("gamma[0,0] against v", U1["gamma[0,0]"], U1["v"]),
            ("Phi[0] against v", U1["Phi[0]"], U1["v"])]
    for site in ("gamma[2,0]", "gamma[1,2]", "Phi[1]", "v"):
        duos.append((f"{site} at iterations 1 and 2", U1[site], U2[site]))
        duos.append((f"{site} in chains c and c + 1", U1[site][0::2], U1[site][1::2]))
    return [(name,) + H.pair_counts(a, b) for name, a, b in duos]


def check_independence(st, out1, out2, where=""):
    count = 0
    for name, obs, exp in independence_statistics(st, out1, out2):
        p, bins = E.chi2_pvalue(obs, exp)
        print(f"{where} {name}: p = {p:.3g} over {bins} cells")
        assert bins == 16 and p >= E.P_FLOOR, (where, name, p)
        count += 1
    return count


# measured on the oracle: 19 tables, p = 0.096 ... 0.99
def test_draws_are_independent(O):
    st = CASES["main"]
    print("statistical assertions:", check_independence(st, run_oracle(O, st, it=1), run_oracle(O, st, it=2)))


@pytest.mark.parametrize("wrong", H.WRONG_LAWS)
def test_a_wrong_law_is_rejected(O, wrong):
    """The statistics must be able to tell: the oracle's draws of the main case against five deliberately wrong laws -- (1) no boost
    below shape 1, (2) gamma's beta* from the un-rescaled table, (3) the sign of r log beta* flipped, (4) v against the Z from before
    the Phi update, (5) the prior of M read as Gamma(2, scale 4) -- must each fall below P_FLOOR at some site.  (A law that differs
    only by using M where M' is due in gamma's shape is NOT told apart at this C, and is not claimed.)"""
    st = CASES["main"]
    out = run_oracle(O, st)
    if wrong == "M_prior_scale_4":
        ps = dict(m_statistics(st, out, prior_scale=4.0))
    else:
        U, floors, _ = H.step_transforms(st, out, wrong=wrong)
        ps = uniformity(U, floors, wrong)
    name = min(ps, key=ps.get)
    print(f"{wrong}: smallest p = {ps[name]:.3g} at {name}")
    assert ps[name] < E.P_FLOOR, f"C = {C} chains of this case cannot tell the law from '{wrong}'"


INIT_CASES = [(12, 3, 3), (12, 3, 2), (80, 64, 1)]       # N = 64: shape 1 / 64, where most of a draw's mass lies below eps


def check_init(n, N, K, out, where=""):
    Cn = len(out["v"])
    assert (out["M"] == 2.0).all() and (out["order"] == np.arange(1, n + 1)).all()
    # gamma0 is kept as log(gamma) (src/pmdi.jl:75-79) and read back through exp: |log gamma| <= 745 units in the last place
    assert np.allclose(out["gamma0"], out["gamma"], rtol=1e-12, atol=0)
    if K == 1:
        assert (out["Phi"] == 0.0).all()
    U, floors, Z, s_tables = H.init_transforms(n, {**out, "gamma0": out["gamma"]})
    assert np.allclose(out["Z"], Z, rtol=RTOL_Z, atol=0)
    count = 0
    for name, p in uniformity(U, floors, where).items():
        assert p >= E.P_FLOOR, (where, name, p)
        count += 1
    # every gamma0 site at once: N K times the sample, for what is too small to see at one site
    pooled = np.concatenate([u for name, u in U.items() if name.startswith("gamma0")])
    obs, exp = H.uniform_counts(pooled, BINS, max(floors.values()))
    p, bins = E.chi2_pvalue(obs, exp)
    print(f"{where} gamma0, all {N * K} sites pooled: p = {p:.3g} over {bins} bins")
    assert bins >= BINS // 2 and p >= E.P_FLOOR, (where, "gamma0 pooled", p)
    count += 1
    for k, (obs, exp) in enumerate(s_tables):
        p, bins = E.chi2_pvalue(obs, exp)
        print(f"{where} s[:, {k}] over {bins} labels, {int(obs.sum())} draws of {Cn} chains: p = {p:.3g}")
        assert bins >= 2 and p >= E.P_FLOOR, (where, k, p)
        count += 1
    return count


# measured on the oracle: (12, 3, 3) sites 0.049 ... 0.94, pooled 0.67, s 0.24 ... 1.0; (12, 3, 2) sites 0.14 ... 0.94, pooled 0.39,
# s 0.58, 1.0; (80, 64, 1) 65 sites 0.029 ... 0.95 (20 bins: u < 0.40 is one bin, see H.uniform_counts), pooled 0.31, s 0.97
@pytest.mark.parametrize("n,N,K", INIT_CASES)
def test_initial_state_follows_its_laws(O, n, N, K):
    """src/pmdi.jl:59-66,95-96.  The label counts of s are sums over chains of multinomials with each chain's own gamma0 / sum: their
    Pearson statistic is stochastically smaller than the chi-square law it is compared with, so a correct draw fails less often than
    p says, while a label read one slot off moves whole chains' counts and is seen at once."""
    print("statistical assertions:", check_init(n, N, K, run_oracle_init(O, n, N, K), f"n{n} N{N} K{K}"))


# allocations that agree only in part, Phi between 0.5 and 1: many proposals are accepted with a probability well inside (0, 1)
S_ALIGN = np.array([[1, 2, 1], [1, 2, 3], [1, 1, 1], [2, 1, 2], [2, 1, 2], [2, 3, 1], [3, 3, 3], [3, 2, 3], [1, 3, 2], [2, 2, 1],
                    [3, 1, 3], [1, 2, 2]])
ALIGN_CASES = {
    "K2": H.State(S_ALIGN[:, :2], G_MAIN[:, :2], G0_MAIN[:, :2], M=(2.0, 2.0), Phi=(0.7,), v=1.0),
    "K3": H.State(S_ALIGN, G_MAIN, G0_MAIN, M=(2.0, 2.0, 2.0), Phi=(0.6, 0.9, 0.5), v=1.0),
    "K3-empty-label": H.State(np.minimum(S_ALIGN, [3, 2, 3]), G_MAIN, G0_MAIN, M=(2.0, 2.0, 2.0), Phi=(1.0, 0.5, 0.8), v=1.0),
}


def check_align(st, out, where=""):
    law, reached = H.align_law(st.s, st.Phi, st.N)
    inside = [a for a, p in reached if 0.05 < a < 0.95 and p > 0.01]
    print(f"{where}: {len(law)} outcomes, {len(reached)} proposals reached, {len(inside)} of them accepted with 0.05 < probability < 0.95")
    assert len(inside) >= 6 and len(law) >= 8, "the case does not exercise the acceptance rule"
    keys = sorted(law)
    index = {key: i for i, key in enumerate(keys)}
    got = H.align_outcomes(st.s, st.gamma, out["s"], out["gamma"])
    assert all(g in index for g in got), "an outcome the reference cannot produce"
    obs = np.bincount([index[g] for g in got], minlength=len(keys))
    p, bins = E.chi2_pvalue(obs, np.array([law[key] for key in keys]) * len(got))
    print(f"{where}: p = {p:.3g} over {bins} bins")
    assert bins >= 6 and p >= E.P_FLOOR, (where, p)
    return 1


# measured on the oracle: K2 p = 0.17 (21 bins), K3 0.64 (22 bins), K3-empty-label 0.76 (29 bins)
@pytest.mark.parametrize("name", list(ALIGN_CASES))
def test_align_labels_follows_its_enumerated_law(O, name):
    st = ALIGN_CASES[name]
    check_align(st, run_oracle_align(O, st), name)
