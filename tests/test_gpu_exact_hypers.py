"""The HIP kernels of csrc/pmdi_hypers.hip (gibbs_init_kernel, hypers_kernel, align_kernel) against the closed-form laws of
tests/_exact_hypers.py: the cases, seeds, chain counts, bins and bounds of tests/test_exact_hypers.py (which asks the same of the
oracle on the CPU), with the C = 4096 chains of a case as the chains of one Gibbs handle.  Nothing here is compared with the oracle.

The statistical assertions are those of tests/test_exact_hypers.py without its five-wrong-laws test: 175 at p >= 1e-6, so correct
kernels fail one with probability about 1.8e-4, and never again once these seeds have been seen to pass.
"""
import numpy as np
import pytest

import test_exact_hypers as T

pytestmark = pytest.mark.gpu

P = 32                   # particles: the hyper-parameter kernels do not look at them


def make(pkg, n, N, K, chains=T.C, seed=T.SEED):
    rng = np.random.default_rng(1)
    sw = pkg.Sweeper([rng.normal(size=(n, 2)) for _ in range(K)], ["gaussian"] * K, N, P, n_chains=chains, seed=seed)
    return sw, pkg.Gibbs(sw, rho=0.25)


def read(g, chains, keys):
    got = [g.get(c) for c in range(chains)]
    return {key: np.array([st[key] for st in got]) for key in keys}


def put(g, st, chains):
    for c in range(chains):
        g.set(c, M=st.M, gamma=st.gamma, gamma0=st.gamma0, Phi=st.Phi, v=st.v, Z=1.0, s=st.s, order=st.order)


STEP_KEYS = ("M", "gamma", "Phi", "v", "Z", "order", "s")


def run_gpu(pkg, st, iterations=1):
    """`iterations` times: the state st into every chain, STEP_BEGIN, STEP_HYPERS (iteration keys 1, 2, ...) -> list of outputs."""
    sw, g = make(pkg, st.n, st.N, st.K)
    try:
        outs = []
        for _ in range(iterations):
            put(g, st, T.C)
            g.step(pkg.STEP_BEGIN); g.step(pkg.STEP_HYPERS)
            outs.append(read(g, T.C, STEP_KEYS))
        return outs
    finally:
        g.close(); sw.close()


@pytest.mark.parametrize("name", list(T.CASES))
def test_one_step_follows_the_closed_form_laws(pkg, name):
    st = T.CASES[name]
    print("statistical assertions:", T.check_step(st, run_gpu(pkg, st)[0], T.SHUFFLE_GROUP[name], name))


def test_draws_are_independent(pkg):
    st = T.CASES["main"]
    out1, out2 = run_gpu(pkg, st, iterations=2)
    print("statistical assertions:", T.check_independence(st, out1, out2))


@pytest.mark.parametrize("n,N,K", T.INIT_CASES)
def test_initial_state_follows_its_laws(pkg, n, N, K):
    sw, g = make(pkg, n, N, K)
    try:
        out = read(g, T.C, ("M", "gamma", "gamma0", "Phi", "v", "Z", "order", "s"))
    finally:
        g.close(); sw.close()
    print("statistical assertions:", T.check_init(n, N, K, out, f"n{n} N{N} K{K}"))


@pytest.mark.parametrize("name", list(T.ALIGN_CASES))
def test_align_labels_follows_its_enumerated_law(pkg, name):
    st = T.ALIGN_CASES[name]
    sw, g = make(pkg, st.n, st.N, st.K)
    try:
        put(g, st, T.C)
        g.step(pkg.STEP_BEGIN); g.step(pkg.STEP_ALIGN)
        out = read(g, T.C, ("gamma", "s"))
    finally:
        g.close(); sw.close()
    T.check_align(st, out, name)
