"""Reduced cluster pools (pmdi_config::pool_cap < N*P+1, what bench.py runs with) at the exact PMDI_E_POOL boundary, on every form of
the sweep.  need = the oracle's stats["max_id"] of the sweep (the largest id any step of any dataset touched): a handle with
pool_cap = need must give the oracle's sweep in everything, one with need - 1 must stop the chain with PMDI_E_POOL -- that chain
only, keeping its input labels -- and the next sweep of the same handle from inputs that fit must be the oracle's again."""
import ctypes as C

import numpy as np
import pytest

from _cases import check_state_cap, check_work_counters, pool_need, t5_invariants
from conftest import random_hypers

pytestmark = pytest.mark.gpu


def _planted(rng, n, K, D=8, sep=3.0):
    z = rng.integers(0, 3, n)
    return [rng.normal(size=(n, D + k)) + sep * (z[:, None] - 1) for k in range(K)], z


def _mixed(rng, n):
    """Gaussian, Categorical, NegBinom datasets sharing a planted 3-cluster structure."""
    z = rng.integers(0, 3, n)
    g = rng.normal(size=(n, 8)) + 3.0 * (z[:, None] - 1)
    c = 1 + (rng.random((n, 6)) < (0.15 + 0.35 * z[:, None])).astype(np.int64) + (z[:, None] == 2) * rng.integers(0, 2, (n, 6))
    nb = rng.geometric(0.2 + 0.25 * z[:, None], size=(n, 5)) - 1
    return [g, c, nb], ["gaussian", "categorical", "negbinom"], z


def _inputs(rng, n, K, N, z=None, scramble=0.0, settle=0.0):
    """Random labels (z None: the start of src/pmdi.jl:63-66) or the planted clustering with a fraction scrambled; order, Pi, Phi."""
    if z is None:
        s = rng.integers(1, N + 1, size=(n, K))
    else:
        s = np.repeat((z + 1)[:, None], K, axis=1)
        idx = rng.random((n, K)) < scramble
        s[idx] = rng.integers(1, N + 1, size=int(idx.sum()))
    Pi, Phi = random_hypers(rng, N, K)
    if settle:
        Pi[:3] += settle; Pi /= Pi.sum(0)
    return s, rng.permutation(n) + 1, Pi, Phi


def _oracle(O, data, kinds, N, P, seed, it, inp, n1):
    n = data[0].shape[0]
    o = O.Oracle(data, kinds, N, P, seed=seed)
    rec = o.debug_steps(n - n1 + 1)
    ro = o.sweep(it, inp[0], inp[1], n1, inp[2], inp[3], trace=True)
    out = ro, rec, o.work(), o.export()
    o.close()
    return out


def _sweep1(sw, it, inp, n1):
    return sw.sweep(it, inp[0][None], inp[1][None], n1, inp[2][None], np.atleast_1d(inp[3])[None], trace=True)


def _equal(sw, rg, want, c, N, n, live_only=False):
    """Everything test_gpu_sweep._compare_run asserts for chain c, plus the cap-aware exported state and the T5 invariants at cap."""
    ro, rec, (up, mv), eo = want
    K = sw.K
    bad = np.where(~np.isclose(rg["trace"][c], ro["trace"], rtol=1e-9, atol=1e-9).all(axis=1))[0]
    assert bad.size == 0, f"first diverging swept observation: {bad[0]} gpu={rg['trace'][c][bad[0]]} cpu={ro['trace'][bad[0]]}"
    assert (rg["s"][c] == ro["s"]).all() and int(rg["p_star"][c]) == ro["p_star"]
    assert np.allclose(rg["logweight"][c], ro["logweight"], rtol=1e-9, atol=1e-8)
    for key in ("n_operations", "n_resamples", "n_clones", "max_id", "sum_classes"):
        assert rg["stats"][c][key] == ro["stats"][key], key
    wk = sw.work_counters()[c]
    assert (wk[:, 1] == up).all() and (wk[:, 3] == mv).all() and wk[:, 2].sum() == ro["stats"]["n_clones"]
    kern = int(sw.swept_by()[c])
    check_work_counters(wk, rec, ro["trace"], N, kern)
    eg = sw.export_state(c)
    # (the settled-chain kernel exports no cluster sizes above max_id: check_state_cap)
    check_state_cap(eg, eo, sw.cap, live_only=live_only or kern != 0)
    t5_invariants(eg, N, sw.P, K, n, cap=sw.cap)
    return kern


def _boundary(pkg, O, data, kinds, N, P, seed, it, inp, n1, refit=None, **kw):
    """cap = need: the oracle's sweep; cap = need - 1: PMDI_E_POOL; then (refit) the failed handle sweeps the first candidate input
    that fits and equals the oracle.  Returns need, the step-path counters and the kernel of the sweep at cap = need."""
    n = data[0].shape[0]
    want = _oracle(O, data, kinds, N, P, seed, it, inp, n1)
    need = pool_need(want[0])
    assert need - 1 >= N + 2, need
    sw = pkg.Sweeper(data, kinds, N, P, n_chains=1, seed=seed, pool_cap=need, **kw)
    assert sw.cap == need
    rg = _sweep1(sw, it, inp, n1)
    kern = _equal(sw, rg, want, 0, N, n)
    paths = {k: rg["stats"][0][k] for k in ("steps_fast", "steps_converted", "steps_fallback")}
    split = sw.split
    sw.close()
    sw = pkg.Sweeper(data, kinds, N, P, n_chains=1, seed=seed, pool_cap=need - 1, **kw)
    assert sw.split == split
    with pytest.raises(pkg.PmdiError) as e:
        _sweep1(sw, it, inp, n1)
    assert e.value.code == -4                                   # PMDI_E_POOL
    if refit:
        for it2, inp2 in refit:
            w2 = _oracle(O, data, kinds, N, P, seed, it2, inp2, n1)
            if pool_need(w2[0]) <= need - 1:
                _equal(sw, _sweep1(sw, it2, inp2, n1), w2, 0, N, n, live_only=True)
                break
        else:
            raise AssertionError(f"no refit candidate needs fewer than {need} ids")
    sw.close()
    return need, paths, kern


def _refit(rng, n, K, N, z, m=3):
    return [(3, _inputs(rng, n, K, N, z, 0.0, 20.0)) for _ in range(m)]


def test_general_kernel_k1_every_block_size(pkg, O, monkeypatch):
    """The general kernel (PMDI_SETTLED=0), K = 1, T = 256 / 512 / 1024 threads: from a random start (census and fallback paths) and
    from a planted one (the unanimous fast path); together the three step paths all occur at cap = need.  Every handle that failed
    sweeps a fitting input next (after the census path, which writes before it decides)."""
    monkeypatch.setenv("PMDI_SETTLED", "0")
    rng = np.random.default_rng(71)
    n, N, P, n1 = 400, 16, 1024, 100
    data, z = _planted(rng, n, 1, D=3, sep=1.5)
    tot = {"steps_fast": 0, "steps_converted": 0, "steps_fallback": 0}
    for block in (256, 512, 1024):
        for start in ("random", "planted"):
            inp = _inputs(rng, n, 1, N, None if start == "random" else z, 0.05, 1.0)
            need, paths, kern = _boundary(pkg, O, data, ["gaussian"], N, P, 72 + block, 2, inp, n1, refit=_refit(rng, n, 1, N, z),
                                          block_threads=block)
            assert kern == 0
            print(f"general K=1 T={block} {start}: need {need}, step paths {paths}")
            for key in tot:
                tot[key] += paths[key]
    assert all(v > 0 for v in tot.values()), tot


@pytest.mark.parametrize("ksplit", [0, 1], ids=["one-workgroup", "split"])
def test_general_kernel_k3_mixed(pkg, O, monkeypatch, ksplit):
    """K = 3 mixed cluster types on the general kernel: the K datasets inside one workgroup per chain, and K cooperating workgroups."""
    monkeypatch.setenv("PMDI_SETTLED", "0")
    monkeypatch.setenv("PMDI_KSPLIT", str(ksplit))
    rng = np.random.default_rng(81 + ksplit)
    n, N, P, n1 = 300, 10, 512, 75
    data, kinds, z = _mixed(rng, n)
    sw = pkg.Sweeper(data, kinds, N, P, pool_cap=N + 2)
    assert sw.split == bool(ksplit)
    sw.close()
    for start in ("random", "planted"):
        inp = _inputs(rng, n, 3, N, None if start == "random" else z, 0.05, 1.0)
        need, paths, kern = _boundary(pkg, O, data, kinds, N, P, 83, 2, inp, n1, refit=_refit(rng, n, 3, N, z))
        assert kern == 0
        print(f"general K=3 ksplit={ksplit} {start}: need {need}, step paths {paths}")


@pytest.mark.parametrize("P,N,kinds", [(1024, 8, ("gaussian", "gaussian")), (2048, 12, ("gaussian", "categorical", "negbinom"))],
                         ids=["four-wave", "eight-wave"])
def test_settled_chain_kernel(pkg, O, P, N, kinds):
    """The settled-chain kernel on a planted start, forced (settled = 2, sticky = 0): it sweeps the whole chain (swept_by 1) at
    cap = need, stops it with PMDI_E_POOL at need - 1, and sweeps a fitting input on that handle next."""
    rng = np.random.default_rng(91 + P)
    n, n1 = 240, 60
    kinds = list(kinds)
    K = len(kinds)
    if K == 3:
        data, kinds, z = _mixed(rng, n)
    else:
        data, z = _planted(rng, n, K)
    tun = {"settled": 2, "sticky": 0, "ksplit": 0}
    found = []
    for j in range(3):         # (an input whose steps outgrow the kernel's tables is handed over: compared all the same, next one)
        inp = _inputs(rng, n, K, N, z, 0.03, 5.0)
        need, _, kern = _boundary(pkg, O, data, kinds, N, P, 93, 2 + j, inp, n1, refit=_refit(rng, n, K, N, z), tuning=tun)
        found.append((need, kern))
        if kern == 1:
            break
    print(f"settled-chain kernel P={P}: (need, swept_by) per tried input {found}")
    assert found[-1][1] == 1, found


def test_hand_over_continuation(pkg, O):
    """The settled-chain kernel handing the chain over mid-sweep to the general kernel's code (classes squeezed to 16; the shape of
    test_hand_over_mid_sweep_equals_oracle[K1]): at cap = need a sweep that was handed over (swept_by 2) equals the oracle, and the
    same inputs at need - 1 stop with PMDI_E_POOL."""
    rng = np.random.default_rng(305)
    n, N, P, n1 = 260, 40, 512, 65
    data, z = _planted(rng, n, 1, D=9)
    tun = {"settled": 2, "sticky": 0, "ksplit": 0, "s2_cls": 16}
    found = []
    # (scrambled fraction, prior mass on three labels): the last one fans out into more than 16 classes at its second swept step and
    # reaches its largest id only about 100 steps later -- the continuation takes the chain to the boundary
    for j, (scramble, settle) in enumerate(((0.08, 0.0), (0.08, 0.1), (0.15, 0.0), (0.3, 0.0))):
        inp = _inputs(rng, n, 1, N, z, scramble, settle)
        need, _, kern = _boundary(pkg, O, data, ["gaussian"], N, P, 903, 2 + j, inp, n1, tuning=tun)
        found.append((need, kern))
        if kern == 2:
            break
    print(f"hand-over: (need, swept_by) per tried input {found}")
    assert found[-1][1] == 2, found


def _many_chains(pkg, O, monkeypatch, settled):
    """Eight chains with different seeds and inputs in one launch, cap = their (lower) median need."""
    import torch
    from particlemdi_jl_amd._lib import _check, lib
    rng = np.random.default_rng(111 + settled)
    n, N, P, K, Cn, n1 = 240, 8, 1024, 2, 8, 60
    data, z = _planted(rng, n, K)
    kinds = ["gaussian"] * K
    if settled:
        tun = {"settled": 2, "sticky": 0, "ksplit": 0}
        # odd chains scrambled more: they need more ids, and every one of them but the last has neighbours on both sides
        inps = [_inputs(rng, n, K, N, z, 0.02 if c % 2 == 0 else 0.06, 5.0) for c in range(Cn)]
    else:
        monkeypatch.setenv("PMDI_SETTLED", "0")
        monkeypatch.setenv("PMDI_KSPLIT", "0")
        tun = None
        inps = [_inputs(rng, n, K, N, z if c % 2 == 0 else None, 0.05, 1.0) for c in range(Cn)]
    seed, it = 120, 2
    wants = [_oracle(O, data, kinds, N, P, seed + c, it, inps[c], n1) for c in range(Cn)]
    needs = np.array([pool_need(w[0]) for w in wants])
    cap = int(np.sort(needs)[Cn // 2 - 1])
    fits = needs <= cap
    print(f"{'settled-chain' if settled else 'general'} x {Cn}: needs {needs.tolist()}, cap {cap}")
    assert fits.any() and not fits.all()
    assert any(not fits[c] for c in range(1, Cn - 1))          # a failing chain with neighbours on both sides
    sw = pkg.Sweeper(data, kinds, N, P, n_chains=Cn, seed=seed, pool_cap=cap, block_threads=0 if settled else 1024, tuning=tun)
    assert not sw.split and sw.settled == bool(settled)
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
    s_in = np.stack([i[0].T - 1 for i in inps])
    s_d = t(s_in, torch.int32); o_d = t(np.stack([i[1] - 1 for i in inps]), torch.int32)
    Pi_d = t(np.stack([i[2].T for i in inps]), torch.float64); lp_d = t(np.stack([np.log(1.0 + i[3]) for i in inps]), torch.float64)
    so = torch.full_like(s_d, -1); lw = torch.empty((Cn, P), dtype=torch.float64, device=dev)
    ps = torch.empty(Cn, dtype=torch.int32, device=dev); st = torch.zeros((Cn, 8), dtype=torch.int64, device=dev)
    er = torch.ones(Cn, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev)
    p = lambda x: C.c_void_p(x.data_ptr())
    _check(lib().pmdi_sweep_device(sw.h, it, p(s_d), p(o_d), n1, p(Pi_d), p(lp_d), None, 1.0, p(so), p(lw), p(ps), p(st), p(er),
                                   C.c_void_p(stream.cuda_stream)))
    torch.cuda.synchronize()
    er, so, ps, st, lw = er.cpu().numpy(), so.cpu().numpy(), ps.cpu().numpy(), st.cpu().numpy(), lw.cpu().numpy()
    by = sw.swept_by()
    for c in range(Cn):
        ro, _, _, eo = wants[c]
        if fits[c]:
            assert er[c] == 0, (c, er[c], needs[c], cap)
            assert (so[c].T + 1 == ro["s"]).all() and int(ps[c]) + 1 == ro["p_star"]
            assert np.allclose(lw[c], ro["logweight"], rtol=1e-9, atol=1e-8)
            for j, key in enumerate(("n_operations", "n_resamples", "n_clones", "max_id", "sum_classes")):
                assert st[c, j] == ro["stats"][key], (c, key)
            check_state_cap(sw.export_state(c), eo, cap, live_only=bool(settled))
            assert int(by[c]) in ((1, 2) if settled else (0,)), (c, by[c])
        else:
            assert er[c] == -4, (c, er[c], needs[c], cap)         # PMDI_E_POOL in its own slot
            assert (so[c] == s_in[c]).all()                        # ... keeping its input labels
    if settled:
        assert (by[fits] == 1).any(), by
    print(f"swept_by {by.tolist()}, err {er.tolist()}")
    sw.close()


@pytest.mark.parametrize("settled", [0, 1], ids=["general", "settled-chain"])
def test_many_chains_in_one_launch(pkg, O, monkeypatch, settled):
    _many_chains(pkg, O, monkeypatch, settled)


def test_headline_operating_point(pkg, O):
    """HL as bench.py runs it: pool_cap = 0.4 (N*P+1), hundreds of chains dealt to the three launch groups.  After a short burn-in one
    whole iteration of three chains that stayed within the pool is compared with the oracle (the chains of
    test_headline_shape_many_chains_three_launch_groups, among those whose err stayed 0); err == 0 exactly where need <= cap."""
    from particlemdi_jl_amd import workloads
    from test_gpu_full import _one_iteration_vs_oracle
    w = workloads.make("HL")
    N, P = w["N"], w["P"]
    cap = max(N + 2, int(0.4 * (N * P + 1)))
    base_seed, C_, burn = 77, 640, 4
    sw = pkg.Sweeper(w["data"], w["kinds"], N, P, n_chains=C_, seed=base_seed, pool_cap=cap)
    assert not sw.split and sw.cap == cap
    g = pkg.Gibbs(sw, rho=0.25)
    g.iterate(burn)
    res = g.results(check=False)
    ok = res["err"] == 0
    print(f"HL x {C_} chains at pool_cap {cap}: {int((~ok).sum())} chains ran out of ids during burn-in")
    assert ok.sum() >= 3
    stats, costs = res["stats"], sw.chain_costs()
    cand = np.where(ok)[0]
    chains = sorted({int(cand[np.argmax(stats[cand, 1])]), int(cand[np.argmax(costs[cand])]), int(cand[np.argsort(costs[cand])[len(cand) // 2]])})
    out = _one_iteration_vs_oracle(pkg, O, w, sw, g, chains, burn + 1, base_seed, False, f"HL x {C_} chains, pool_cap {cap}", cap=cap)
    assert out
    print(f"HL compared chains {sorted(out)}: need {[pool_need(out[c]) for c in sorted(out)]}, kernels {[out[c]['kernel'] for c in sorted(out)]}")
    g.close(); sw.close()
