"""The relabelling accumulator without a GPU: the new entry points are declared, exported and listed; the kernels are in the
code object and compile for gfx950 without scratch; pmdi_relabel_create validates before it touches a device and
pmdi_pooled(relabel=...) checks its pivot first; the assignment loop of tests/_np_relabel.py has the optimal value of
scipy.optimize.linear_sum_assignment on every family of matrices; the arithmetic of AllocationProbabilities on hand-worked counts."""
import ctypes as C
import importlib
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import _np_relabel as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_FUNCTIONS = ["pmdi_relabel_create", "pmdi_relabel_destroy", "pmdi_relabel_reset", "pmdi_relabel_set_pivot", "pmdi_relabel_set_budget",
                 "pmdi_relabel_add_gibbs", "pmdi_relabel_add_arrays", "pmdi_relabel_samples", "pmdi_relabel_get", "pmdi_relabel_last",
                 "pmdi_relabel_assign_device", "pmdi_gibbs_run9"]
KERNELS = ("relabel_rows_kernel", "relabel_table_kernel", "relabel_assign_kernel", "relabel_count_kernel", "relabel_finish_kernel")


def test_new_entry_points_are_declared_exported_and_listed(pkg):
    src = open(os.path.join(ROOT, "include", "pmdi_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(pmdi_[A-Za-z_0-9]+)\s*\(", src))
    lib = pkg.lib()
    for name in NEW_FUNCTIONS:
        assert name in declared, f"{name} is not declared in include/pmdi_hip.h"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in pkg.EXPORTS, f"{name} is not listed in EXPORTS"
    assert lib.pmdi_abi_version() == pkg.ABI_VERSION == 2
    assert re.search(r"#define\s+PMDI_ABI_VERSION\s+2\b", src)
    blob = open(pkg.LIB_PATH, "rb").read()
    for kernel in KERNELS:
        assert kernel.encode() in blob, kernel
    for name in ("RelabelAccumulator", "AllocationProbabilities", "allocation_probabilities", "assign_labels"):
        assert hasattr(pkg, name), name
    relabel = importlib.import_module("particlemdi_jl_amd.relabel")
    assert [relabel.count_tile(N) for N in (2, 128, 129, 255)] == [256, 256, 128, 128]
    # N x tile int32 counts and the staged permutations of 32 chains fit the 160 KiB of LDS
    assert all(4 * N * relabel.count_tile(N) + 32 * N <= 160 * 1024 for N in range(2, 256))


GOOD = dict(n_chains=4, K=2, N=6, n=100, pivot=None, shared=1)


def _create(pkg, a):
    pivot = a["pivot"]
    if pivot is None:
        pivot = np.arange(max(a["K"], 1) * max(a["n"], 1), dtype=np.int32) % 2
    pivot = np.ascontiguousarray(pivot, dtype=np.int32)
    h = C.c_void_p()
    rc = pkg.lib().pmdi_relabel_create(0, a["n_chains"], a["K"], a["N"], a["n"], pivot.ctypes.data_as(C.c_void_p), a["shared"], C.byref(h))
    return rc, h


def _pivot_with(value, at=157):
    pivot = np.zeros(200, dtype=np.int32)
    pivot[at] = value
    return pivot


@pytest.mark.parametrize("change", [dict(K=0), dict(K=9), dict(N=1), dict(N=256), dict(n=0), dict(n=65536), dict(n_chains=0),
                                    dict(pivot=_pivot_with(-2)), dict(pivot=_pivot_with(6)), dict(pivot=_pivot_with(6, at=0)),
                                    dict(shared=2), dict(shared=-1)], ids=str)
def test_create_validates_before_any_device_use(pkg, change):
    rc, h = _create(pkg, {**GOOD, **change})
    assert rc == -1                    # PMDI_E_ARG, with or without a GPU
    assert not h.value
    assert b"pivot" in pkg.lib().pmdi_last_error() or "pivot" not in change


def test_create_with_good_arguments_reaches_the_device(pkg):
    """The checks above are not vacuous: the same call with nothing wrong gets as far as the device -- PMDI_E_DEVICE where
    there is none (no CPU path), an accumulator where there is one.  The limits themselves are good arguments: -1 and N - 1."""
    import torch
    edge = _pivot_with(5)
    edge[3] = -1
    for a in (GOOD, {**GOOD, "pivot": edge}, {**GOOD, "K": 8, "N": 2, "n": 65535, "n_chains": 1, "shared": 0}, {**GOOD, "K": 1, "N": 255, "n": 1}):
        rc, h = _create(pkg, a)
        if torch.cuda.is_available():
            assert rc == 0 and h.value
            assert pkg.lib().pmdi_relabel_samples(h) == 0
            assert pkg.lib().pmdi_relabel_destroy(h) == 0
        else:
            assert rc == -2 and not h.value
    assert pkg.lib().pmdi_relabel_samples(None) == 0
    assert pkg.lib().pmdi_relabel_destroy(None) == 0


def test_null_handles_and_bad_solver_arguments_are_argument_errors(pkg):
    lib = pkg.lib()
    assert lib.pmdi_relabel_create(0, 1, 2, 2, 1, None, 1, C.byref(C.c_void_p())) == -1
    assert lib.pmdi_relabel_create(0, 1, 2, 2, 1, None, 1, None) == -1
    assert lib.pmdi_relabel_reset(None, None) == -1
    assert lib.pmdi_relabel_set_pivot(None, None, None) == -1
    assert lib.pmdi_relabel_set_budget(None, 1) == -1
    assert lib.pmdi_relabel_add_gibbs(None, None, None) == -1
    assert lib.pmdi_relabel_add_arrays(None, None, None, None) == -1
    assert lib.pmdi_relabel_get(None, *([None] * 5), None) == -1
    assert lib.pmdi_relabel_last(None, None, None, None) == -1
    assert lib.pmdi_gibbs_run9(None, 1, 0, 1, *([None] * 9), None) == -1
    for B, N in ((-1, 5), (1 << 31, 5), (1, 1), (1, 256)):
        assert lib.pmdi_relabel_assign_device(0, None, B, N, None, None, None) == -1
    assert lib.pmdi_relabel_assign_device(0, None, 1, 5, None, None, None) == -1          # null arrays
    assert lib.pmdi_relabel_assign_device(0, None, 0, 5, None, None, None) == 0           # nothing to do, no device


def test_pmdi_pooled_takes_the_pivot_after_its_checks(pkg, monkeypatch):
    P = importlib.import_module("particlemdi_jl_amd.pmdi")

    class Reached(Exception):
        pass

    def reached(*a, **k):
        raise Reached()
    monkeypatch.setattr(P, "Sweeper", reached)
    x = np.zeros((10, 2))
    two = dict(dataFiles=[x, x], dataTypes=["gaussian", "gaussian"], N=3, particles=4, rho=0.25, iter=5, n_chains=2)
    pivot = np.array([0, 1, 2, -1, -1, 0, 1, 2, 2, 0])
    for value, more in ((pivot, {}), (np.stack([pivot, pivot[::-1]]), {}), (pivot.tolist(), {}), (pivot, {"relabel_shared": False}),
                        (None, {})):
        with pytest.raises(Reached):
            P.pmdi_pooled(**two, relabel=value, **more)
    for value, more in ((pivot[:-1], {}), (np.stack([pivot] * 3), {}), (np.zeros((2, 2, 10), dtype=int), {}), (pivot.astype(float), {}),
                        (pivot == 0, {}), (np.where(pivot == 2, 3, pivot), {}), (np.where(pivot == 2, -2, pivot), {}), ("consensus", {}),
                        (True, {}), (1, {}), (pivot, {"relabel_shared": 1}), (pivot, {"relabel_shared": "yes"}), (None, {"relabel_shared": True})):
        with pytest.raises(ValueError):
            P.pmdi_pooled(**two, relabel=value, **more)


def test_the_readme_example_passes_the_checks(pkg, monkeypatch):
    """The README's pmdi_pooled(..., relabel=...) line gets as far as Sweeper with a pivot that leaves observations out."""
    P = importlib.import_module("particlemdi_jl_amd.pmdi")
    text = open(os.path.join(ROOT, "README.md")).read()
    calls = [m for m in re.findall(r"pmdi_pooled\(([^\n]*)\)", text) if "relabel=" in m]
    assert len(calls) == 1, calls
    kw = {k: int(v) for k, v in re.findall(r"\b(N|particles|iter|n_chains|burnin|thin)=(\d+)", calls[0])}
    assert sorted(kw) == ["N", "burnin", "iter", "n_chains", "particles", "thin"] and "relabel=pivot" in calls[0]

    class Reached(Exception):
        pass

    def reached(*a, **k):
        raise Reached()
    monkeypatch.setattr(P, "Sweeper", reached)
    x = np.zeros((100, 2))
    pivot = np.where(np.arange(100) % 7 == 0, -1, np.arange(100) % 4)
    with pytest.raises(Reached):
        P.pmdi_pooled([x] * 4, ["GaussianCluster"] * 4, rho=0.25, relabel=pivot, **kw)


# ---- the checker's assignment loop ----
def _optimum(W):
    from scipy.optimize import linear_sum_assignment
    r, c = linear_sum_assignment(np.asarray(W), maximize=True)
    return int(np.asarray(W, dtype=np.int64)[r, c].sum())


@pytest.mark.parametrize("family", ["ties", "zero", "large", "negative", "noisy"])
def test_the_loop_has_the_optimal_value(family):
    """80 matrices of each family, N = 2..39 (the 400 of the issue): a permutation with scipy's optimal value; both forms of
    the loop give the same permutation."""
    rng = np.random.default_rng(["ties", "zero", "large", "negative", "noisy"].index(family))
    for t in range(80):
        N = 2 + (t * 37 + 11) % 38
        W = X.matrix_families(rng, N)[family]
        sigma, value = X.assign(W)
        assert sorted(sigma) == list(range(N)) and value == _optimum(W), (family, N)
        assert X.assign_np(W) == (sigma, value), (family, N)


def test_the_loop_at_255_labels_with_large_entries():
    rng = np.random.default_rng(255)
    W = rng.integers(0, 524281, (255, 255))
    W[rng.integers(0, 255), rng.integers(0, 255)] = 524280
    sigma, value = X.assign(W)
    assert sorted(sigma) == list(range(255)) and value == _optimum(W)
    assert X.assign_np(W) == (sigma, value)
    ties = rng.integers(0, 3, (255, 255))                 # where the tie-breaks decide: the two forms still agree
    assert X.assign_np(ties) == X.assign(ties) and X.assign(ties)[1] == _optimum(ties)


def test_a_state_equal_to_the_pivot_gives_the_identity():
    rng = np.random.default_rng(7)
    for N, n, K in ((2, 5, 1), (6, 40, 3), (20, 300, 2)):
        pivot = rng.integers(0, N - 1, (K, n))             # the last class stays empty
        for shared in (True, False):
            W = X.tables_of(pivot[None], pivot, N, shared)
            for u in range(W.shape[1]):
                sigma, value = X.assign(W[0, u])
                assert sigma == list(range(N)) and value == (K * n if shared else n)
    # the pivot under other names comes back: sigma undoes the renaming on the occupied labels
    N, n = 7, 60
    pivot = rng.integers(0, N, (1, n))
    ren = rng.permutation(N)
    sigma, value = X.assign(X.tables_of(ren[pivot][None], pivot, N, True)[0, 0])
    assert value == n and all(sigma[ren[g]] == g for g in np.unique(pivot))


def test_the_mirror_by_hand():
    """C = 1, K = 2, N = 3, n = 4, shared: the state is the pivot with labels 0 and 1 exchanged, label 2 unused."""
    pivot = np.array([[0, 0, 1, -1], [0, 1, 1, 1]])
    s = np.array([[[1, 1, 0, 2], [1, 0, 0, 0]]])
    m = X.Mirror(1, 2, 3, 4, pivot, True)
    Pi = np.array([[[0.5, 0.25, 0.25], [0.125, 0.75, 0.125]]])
    m.add(s, Pi)
    assert m.perm.tolist() == [[[1, 0, 2]]] and m.value.tolist() == [[7]] and m.moved.tolist() == [[1]]
    # the observation outside the matching (pivot -1) is counted under its relabelled label all the same
    assert m.alloc[0].tolist() == [[1, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]
    assert m.alloc[1].tolist() == [[1, 0, 0], [0, 1, 0], [0, 1, 0], [0, 1, 0]]
    assert m.w_sum.tolist() == [[[0.25, 0.5, 0.25], [0.75, 0.125, 0.125]]] and m.w_sq[0, 0].tolist() == [0.0625, 0.25, 0.0625]
    m.add(pivot.clip(0)[None])                              # the pivot itself (its -1 as label 0): the identity, nothing moves
    assert m.perm.tolist() == [[[0, 1, 2]]] and m.moved.tolist() == [[1]] and m.match_sum.tolist() == [[14]] and m.T == 2
    assert m.w_sum.tolist() == [[[0.25, 0.5, 0.25], [0.75, 0.125, 0.125]]]          # an add without Pi leaves the weights alone
    # per dataset: dataset 0 sees only labels 1, 0 against 0, 1
    m2 = X.Mirror(1, 2, 3, 4, pivot, False)
    m2.add(s)
    assert m2.perm.tolist() == [[[1, 0, 2], [1, 0, 2]]] and m2.value.tolist() == [[3, 4]]
    s_bad = s.copy()
    s_bad[0, 0, 0] = 3                                      # out of range: in no cell and nowhere in alloc
    m3 = X.Mirror(1, 2, 3, 4, pivot, True)
    m3.add(s_bad)
    assert m3.value.tolist() == [[6]] and m3.alloc[0, 0].tolist() == [0, 0, 0]


# ---- AllocationProbabilities: hand-worked counts ----
def _result(pkg):
    # K = 1, n = 3, N = 3, C = 2 chains of T = 2 draws: 4 draws per observation
    alloc = np.array([[[4, 0, 0], [2, 2, 0], [1, 1, 2]]])
    return pkg.AllocationProbabilities(2, alloc, match_sum=[[6], [3]], moved=[[1], [2]], n_match=[3],
                                       w_sum=[[[1.0, 0.5, 0.5]], [[0.5, 1.0, 0.5]]], w_sq=[[[0.5, 0.125, 0.125]], [[0.125, 0.625, 0.125]]])


def test_allocation_probabilities_by_hand(pkg):
    r = _result(pkg)
    assert (r.T, r.C, r.U, r.K, r.n, r.N) == (2, 2, 1, 1, 3, 3)
    assert r.probabilities().tolist() == [[[1.0, 0.0, 0.0], [0.5, 0.5, 0.0], [0.25, 0.25, 0.5]]]
    assert r.hard().tolist() == [[0, 0, 2]] and r.hard().dtype == np.int32        # the tie of observation 1 goes to the smaller label
    assert r.confidence().tolist() == [[1.0, 0.5, 0.5]]
    assert r.entropy().tolist() == [[0.0, 1.0, 1.5]]
    assert r.uncertain(0.8).tolist() == [[False, True, True]] and r.uncertain(0.5).tolist() == [[False, False, False]]
    assert r.expected_sizes().tolist() == [[1.75, 0.75, 0.5]]
    assert r.weights().tolist() == [[0.375, 0.375, 0.25]]
    assert r.agreement().tolist() == [[1.0], [0.5]] and r.switch_rate().tolist() == [0.75]
    # component 0: chain means 0.5 and 0.25; v_c = (0.5 - 2 / 4) / 1 = 0 and (0.125 - 2 / 16) / 1 = 0: W = 0, NaN
    # component 1: chain means 0.25 and 0.5; v_c = (0.125 - 0.125) = 0 and (0.625 - 0.5) = 0.125: W = 0.0625;
    #   B = 2 var([0.25, 0.5], ddof = 1) = 2 / 32 = 0.0625; R-hat = sqrt(1 / 2 + 0.0625 / 2 / 0.0625) = 1
    rh = r.weights_rhat()
    assert np.isnan(rh[0, 0]) and rh[0, 1] == 1.0 and np.isnan(rh[0, 2])
    x = np.array([[0.0, 4.0], [2.0, 0.0], [4.0, 4.0]])
    # P^T X / sum P: component 0 has P = (1, 0.5, 0.25): (0 + 1 + 1) / 1.75, (4 + 0 + 1) / 1.75
    prof = r.profiles(x, 0)
    assert prof.shape == (3, 2) and prof[0].tolist() == [2.0 / 1.75, 5.0 / 1.75] and prof[2].tolist() == [4.0, 4.0]
    never = pkg.AllocationProbabilities(1, np.array([[[1, 0]]]), [[1]], [[0]], [1])
    assert np.isnan(never.profiles(np.ones((1, 2)), 0)[1]).all()
    for call in (never.weights, never.weights_rhat):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        pkg.AllocationProbabilities(0, np.zeros((1, 1, 2)), [[0]], [[0]], [1]).probabilities()
    with pytest.raises(ValueError):
        r.profiles(x[:2], 0)
    with pytest.raises(ValueError):
        r.uncertain(0.0)


def test_merge_adds_alloc_and_concatenates_the_chains(pkg):
    a, b = _result(pkg), _result(pkg)
    b.alloc = b.alloc[:, ::-1].copy()
    m = a.merge(b)
    assert (m.T, m.C, m.U) == (2, 4, 1) and np.array_equal(m.alloc, a.alloc + b.alloc)
    assert m.match_sum.tolist() == [[6], [3], [6], [3]] and m.w_sum.shape == (4, 1, 3)
    assert m.probabilities().sum(axis=2).tolist() == [[1.0, 1.0, 1.0]]
    assert m.agreement()[:, 0].tolist() == [1.0, 0.5, 1.0, 0.5] and m.switch_rate().tolist() == [0.75]
    other = pkg.AllocationProbabilities(3, a.alloc, a.match_sum, a.moved, [3])
    with pytest.raises(ValueError):
        a.merge(other)
    no_weights = pkg.AllocationProbabilities(2, a.alloc, a.match_sum, a.moved, [3])
    assert a.merge(no_weights).w_sum is None


# ---- the kernels' build ----
def test_relabel_kernels_use_no_scratch():
    """hipcc cross-compiles without a GPU: every kernel of pmdi_relabel.hip -- the two builds of the table kernel and the four
    of the solver (one, two, four columns per lane; the cost matrix in LDS or not) -- reports ScratchSize 0 and no spills."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "particlemdi.jl_amd", "csrc", "pmdi_relabel.hip")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC",
                            "--cuda-device-only", "-c", src, "-o", os.path.join(tmp, "x.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    cur, scratch, vspill = None, {}, {}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            scratch[cur] = int(m.group(1))
        m = re.search(r"VGPRs Spill: (\d+)", line)
        if m and cur:
            vspill[cur] = int(m.group(1))
    assert len([k for k in scratch if "relabel_table_kernel" in k]) == 2, sorted(scratch)
    assert len([k for k in scratch if "relabel_assign_kernel" in k]) == 4, sorted(scratch)
    for want in KERNELS:
        assert any(want in k for k in scratch), (want, sorted(scratch))
    for k in scratch:
        assert scratch[k] == 0 and vspill[k] == 0, (k, scratch[k], vspill[k])
