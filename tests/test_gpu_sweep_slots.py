"""Workgroups of the settled-chain launch that keep their slot (pmdi_tuning hold / sweep_grid; pmdi_s2::sweep_slots in
csrc/pmdi_sweep2_body.h): a workgroup sweeps a chain, draws the next position of the launch order and sweeps that chain in the LDS
the previous one left behind -- its own tables, or the general kernel's layout after a hand-over.  Results never depend on the
knobs, so every comparison here is bit for bit against the one-shot workgroups of hold = 0: allocations, picked particle,
log-weights, the eight stats words, work counters, which kernel finished each chain, the exported state.  sweep_grid makes a handful
of workgroups sweep all chains, so that every one of them carries several -- which a launch of n_chains workgroups on an idle GPU
never would."""
import functools

import numpy as np
import pytest

from _cases import chain_result, check_state_against_oracle, check_sweep_against_oracle
from conftest import random_hypers
from test_gpu_sweep import _gauss_planted, _mixed_planted

pytestmark = pytest.mark.gpu

GAU, CAT = "gaussian", "categorical"
S2 = {"settled": 2, "sticky": 0, "ksplit": 0}       # every chain starts every sweep on the settled-chain kernel
HAND = dict(S2, s2_cls=16)      # ... whose tables hold 16 particle classes per dataset: the random start's busiest steps (17 .. 27) do not fit


class _Shape:
    pass


def _shape(kinds, N, P, n, C, seed, dseed, D=None, mixed=False):
    sh = _Shape()
    sh.kinds, sh.K, sh.N, sh.P, sh.n, sh.C, sh.seed, sh.n1 = list(kinds), len(kinds), N, P, n, C, seed, n // 4       # (rho = 0.25)
    sh.rng = np.random.default_rng(dseed)
    if mixed:
        sh.data, sh.z = _mixed_planted(sh.rng, n, sh.kinds)
    else:
        sh.data, sh.z = _gauss_planted(sh.rng, n, sh.K, D=D)
        sh.data = [x[:, :D] for x in sh.data]            # (every dataset D features)
    return sh


def _planted_inputs(sh, sweeps, settle):
    """Per sweep: the planted clustering with 4 % of the labels scrambled, an order, Pi with prior mass on the three planted labels,
    Phi -- chains that stay within the settled-chain kernel's tables."""
    K, C, n, N, rng = sh.K, sh.C, sh.n, sh.N, sh.rng
    out = []
    for _ in range(sweeps):
        s = np.repeat(np.repeat((sh.z + 1)[None, :, None], K, axis=2), C, axis=0)
        idx = rng.random(s.shape) < 0.04
        s[idx] = rng.integers(1, N + 1, size=int(idx.sum()))
        hyp = [random_hypers(rng, N, K) for _ in range(C)]
        for h in hyp:
            h[0][:3] += settle; h[0][:] = h[0] / h[0].sum(0)
        out.append((s, np.stack([rng.permutation(n) + 1 for _ in range(C)]), np.stack([h[0] for h in hyp]), np.stack([h[1] for h in hyp])))
    return out


@functools.lru_cache(maxsize=None)
def _random_start():
    """K = 2 Gaussian datasets, 24 chains from the random start of src/pmdi.jl:63-66, four iterations on the oracle (chain c with
    seed + c): the inputs of every sweep, per (sweep, chain) the oracle's result, work counters, per-step record and exported state."""
    import __graft_entry__ as G
    O = G.load_oracle()
    sh = _shape((GAU, GAU), N=6, P=256, n=60, C=24, seed=4100, dseed=41, D=4)
    K, C, n, N, n1, rng = sh.K, sh.C, sh.n, sh.N, sh.n1, sh.rng
    s = rng.integers(1, N + 1, size=(C, n, K))
    orcs = [O.Oracle(sh.data, sh.kinds, N, sh.P, seed=sh.seed + c) for c in range(C)]
    recs = [o.debug_steps(n - n1 + 1) for o in orcs]
    sh.inputs, sh.out = [], []
    for it in range(1, 5):
        order = np.stack([rng.permutation(n) + 1 for _ in range(C)])
        hyp = [random_hypers(rng, N, K) for _ in range(C)]
        sh.inputs.append((s.copy(), order, np.stack([h[0] for h in hyp]), np.stack([h[1] for h in hyp])))
        row = []
        for c in range(C):
            ro = orcs[c].sweep(it, s[c], order[c], n1, hyp[c][0], hyp[c][1], trace=True)
            row.append({"ro": ro, "work": orcs[c].work(), "rec": recs[c].copy(), "state": orcs[c].export()})
            s[c] = ro["s"]
        sh.out.append(row)
    for o in orcs:
        o.close()
    # n_operations per step (a swept observation of one dataset) of every (sweep, chain): what decides a chain's group
    sh.ops = np.array([[x["ro"]["stats"]["n_operations"] for x in row] for row in sh.out]) / ((n - n1 + 1) * K)
    return sh


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _run(pkg, sh, inputs, tuning, trace=False):
    """Sweep `inputs` on a handle with `tuning`.  Returns the handle (the caller closes it), everything the sweeps returned as a list of
    named arrays per sweep, and the raw results per sweep."""
    sw = pkg.Sweeper(sh.data, sh.kinds, sh.N, sh.P, n_chains=sh.C, seed=sh.seed, tuning=tuning)
    got, raw = [], []
    for it, (s, order, Pi, Phi) in enumerate(inputs, start=1):
        rg = sw.sweep(it, s, order, sh.n1, Pi, Phi, trace=trace)
        wk, by = sw.work_counters(), sw.swept_by()
        launch = sw.settled_launch()
        keys = sorted(rg["stats"][0])
        assert len(keys) == 8, keys
        row = {"s": rg["s"], "p_star": rg["p_star"], "logweight": rg["logweight"], "work": wk, "swept_by": by,
               "stats": np.array([[rg["stats"][c][k] for k in keys] for c in range(sh.C)])}
        states = [sw.export_state(c) for c in range(sh.C)]
        for key in ("particle", "counts", "cluster_n", "max_id"):
            row["state." + key] = np.stack([e[key] for e in states])
        got.append(row)
        raw.append({"rg": rg, "wk": wk, "by": by, "states": states, "draws": launch["draws"] if launch else None})
    return sw, got, raw


def _same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        for key in x:
            assert np.array_equal(_bits(x[key]), _bits(y[key])), f"{what}: sweep {i + 1} differs in the bits of {key}"


@functools.lru_cache(maxsize=None)
def _one_shot_random_start(pkg):
    """The reference of case 1: one-shot workgroups (hold = 0), three iterations from the random start."""
    sh = _random_start()
    sw, got, raw = _run(pkg, sh, sh.inputs[:3], dict(HAND, hold=0), trace=True)
    assert sw.settled and sw.settled_launch()["hold"] == 0 and sw.settled_launch()["grid"] == sh.C
    sw.close()
    return got, raw


@pytest.mark.parametrize("grid", [24, 3, 1])
def test_back_to_back_chains_through_hand_overs(pkg, grid):
    """24 chains from the random start, every one on the settled-chain kernel (settled = 2) with tables for 16 particle classes: in
    every sweep a chain or two meets a step with more (the oracle's record: 22; 27 and 17; 17) and is handed over mid-sweep to the
    general kernel's code in the same workgroup -- which then draws its next chain and sweeps it in whatever that code left in the
    LDS.  hold = 2 with 24, 3 and 1 workgroups against hold = 0; some sweep must have both chains the kernel finished itself (1) and
    handed-over ones (2), so with 3 or 1 workgroups a workgroup has swept a chain after carrying a handed-over one; two chains of
    the last sweep against the oracle."""
    sh = _random_start()
    want, want_raw = _one_shot_random_start(pkg)
    kernels = np.stack([r["by"] for r in want_raw])
    print(f"kernels per sweep (1 settled-chain, 2 handed over): {[np.bincount(k, minlength=3).tolist() for k in kernels]}")
    assert set(np.unique(kernels)) <= {1, 2}
    both = [bool((k == 1).any() and (k == 2).any()) for k in kernels]
    assert any(both), kernels
    sw, got, raw = _run(pkg, sh, sh.inputs[:3], dict(HAND, hold=2, sweep_grid=grid), trace=True)
    launch = sw.settled_launch()
    assert (launch["hold"], launch["grid"]) == (2, grid), launch
    # every position of the launch order was drawn (exactly once: the draw is one atomic), then one draw past the end per workgroup
    assert [r["draws"] for r in raw] == [sh.C + grid] * 3, [r["draws"] for r in raw]
    _same(got, want, f"hold=2 sweep_grid={grid} against hold=0")
    it = 3
    last = kernels[it - 1]
    for c in (int(np.flatnonzero(last == 1)[0]) if (last == 1).any() else 0, int(np.flatnonzero(last == 2)[0]) if (last == 2).any() else 1):
        o = sh.out[it - 1][c]
        by = int(raw[it - 1]["by"][c])
        check_sweep_against_oracle(chain_result(raw[it - 1]["rg"], c), o["ro"], raw[it - 1]["wk"][c], o["work"], o["rec"], sh.N, by,
                                   where=f"sweep_grid={grid} chain {c} iteration {it} (kernel {by})")
        check_state_against_oracle(raw[it - 1]["states"][c], o["state"], sh.N, sh.P, sh.K, sh.n)
    sw.close()


def test_headline_instantiation(pkg):
    """K = 4 Gaussian datasets, 1 024 particles: the all-Gaussian four-wave build with four particles per lane that the benchmark
    runs.  Eight planted chains on two workgroups (four chains each on average) against one-shot workgroups."""
    sh = _shape((GAU,) * 4, N=20, P=1024, n=40, C=8, seed=4200, dseed=42, D=5)
    inputs = _planted_inputs(sh, 2, settle=1.0)
    ref, want, want_raw = _run(pkg, sh, inputs, dict(S2, hold=0))
    assert ref.settled and ref.layout()["s2"]["threads"] == 256
    ref.close()
    assert all((r["by"] >= 1).all() for r in want_raw) and any((r["by"] == 1).any() for r in want_raw), [r["by"] for r in want_raw]
    sw, got, raw = _run(pkg, sh, inputs, dict(S2, hold=2, sweep_grid=2))
    assert [r["draws"] for r in raw] == [sh.C + 2] * 2
    _same(got, want, "hold=2 sweep_grid=2 against hold=0")
    sw.close()


def test_eight_wave_build(pkg):
    """2 048 particles: the 512-thread build, Gaussian + Categorical.  Four planted chains on ONE workgroup against one-shot ones."""
    sh = _shape((GAU, CAT), N=8, P=2048, n=30, C=4, seed=4300, dseed=43, mixed=True)
    inputs = _planted_inputs(sh, 2, settle=1.0)
    ref, want, want_raw = _run(pkg, sh, inputs, dict(S2, hold=0))
    assert ref.settled and ref.layout()["s2"]["threads"] == 512
    ref.close()
    assert all((r["by"] >= 1).all() for r in want_raw), [r["by"] for r in want_raw]
    sw, got, raw = _run(pkg, sh, inputs, dict(S2, hold=2, sweep_grid=1))
    assert [r["draws"] for r in raw] == [sh.C + 1] * 2
    _same(got, want, "hold=2 sweep_grid=1 against hold=0")
    sw.close()


def test_automatic_mode_with_both_groups(pkg):
    """hold automatic, default `settled`: the first sweep is the general kernel's; after it a chain is heavy when its last sweep met
    more than light_ids live clusters per step (or was handed over lately).  light_ids = the median of the oracle's n_operations per
    step, so that sweeps 2 .. 4 have chains in both groups -- asserted from the stats the device returned.  The heavy launch's
    workgroups count themselves in, the settled-chain launch's keep their slots from then on; every chain is swept exactly once per
    sweep, by the launch of its group, and everything equals hold = 0 bit for bit."""
    sh = _random_start()
    light_ids = int(np.median(sh.ops))
    steps = (sh.n - sh.n1 + 1) * sh.K
    heavy_next = sh.ops[:-1] > light_ids                    # (sweep, chain): heavy in the NEXT sweep, by the oracle's counters
    assert (heavy_next.sum(axis=1) >= 1).all() and (heavy_next.sum(axis=1) < sh.C).all(), heavy_next.sum(axis=1)
    tuning = {"ksplit": 0, "light_ids": light_ids}
    ref, want, want_raw = _run(pkg, sh, sh.inputs, dict(tuning, hold=0))
    assert ref.settled and ref.settled_launch()["hold"] == 0
    ref.close()
    sw, got, raw = _run(pkg, sh, sh.inputs, tuning)
    launch = sw.settled_launch()
    assert (launch["hold"], launch["grid"]) == (1, sh.C), launch
    for i, r in enumerate(raw):
        ops = np.array([r["rg"]["stats"][c]["n_operations"] for c in range(sh.C)])
        assert (ops == np.round(sh.ops[i] * steps)).all()
        by = r["by"]
        if i == 0:
            assert (by == 0).all(), by                      # the first sweep: every chain is heavy
            continue
        prev = np.array([raw[i - 1]["rg"]["stats"][c]["n_operations"] for c in range(sh.C)])
        handed = np.zeros(sh.C, dtype=bool)
        for j in range(max(0, i - 3), i):                    # (a chain handed over in one of the last three sweeps stays heavy)
            handed |= raw[j]["by"] == 2
        heavy = (prev > light_ids * steps) | handed
        assert heavy.any() and not heavy.all(), (i, heavy)
        # every chain swept once, by the launch of its group: the general kernel's own launch (0) or the settled-chain launch (1, 2)
        assert ((by == 0) == heavy).all(), (i, by, heavy)
        assert sh.C <= r["draws"] <= 2 * sh.C, r["draws"]    # every position of the launch order was drawn
    print(f"light_ids {light_ids}; kernels per sweep {[np.bincount(r['by'], minlength=3).tolist() for r in raw]}; draws {[r['draws'] for r in raw]}")
    _same(got, want, "hold automatic against hold=0")
    sw.close()


def test_one_shot_workgroups_need_a_workgroup_per_chain(pkg):
    sh = _shape((GAU, GAU), N=6, P=256, n=60, C=24, seed=4100, dseed=41, D=4)
    for tuning in (dict(S2, hold=0, sweep_grid=23), dict(S2, hold=0, sweep_grid=1), dict(S2, hold=2, ticket=0, sweep_grid=3)):
        with pytest.raises(pkg.PmdiError) as e:
            pkg.Sweeper(sh.data, sh.kinds, sh.N, sh.P, n_chains=sh.C, seed=sh.seed, tuning=tuning)
        assert e.value.code == -1, e.value            # PMDI_E_ARG
    sw = pkg.Sweeper(sh.data, sh.kinds, sh.N, sh.P, n_chains=sh.C, seed=sh.seed, tuning=dict(S2, hold=0, sweep_grid=24))
    assert sw.settled_launch()["grid"] == 24
    sw.close()
