"""The coupled add of the predictive accumulator without a GPU.  The first tests hold the YARDSTICK, tests/_np_predict_coupled.py
(Python float loops in the order include/pmdi_hip.h states), to a brute-force enumeration of all N^K label tuples and to
properties the joint posterior must have.  The rest run shipped code: the names of the C ABI, the argument errors that come
before any device use, CoupledPredictiveCounts on hand-made counts, and what the compiler reports for the kernels of
pmdi_predict_coupled.hip.
RTOL = 1e-12: every result is a sum of positive terms through at most 3^K + K N 2^K ~ 10^4 roundings, and 10^4 * 2^-53 ~ 1.2e-12."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import _np_predict as X
import _np_predict_coupled as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-12
NEW = ("pmdi_predict_create_coupled", "pmdi_predict_add_arrays_coupled", "pmdi_predict_get_coupled", "pmdi_predict_merge_coupled",
       "pmdi_predict_last_coupled")
CASES = [(2, 3), (3, 4), (4, 5), (5, 3), (8, 2)]


def _case(rng, K, N):
    return rng.random((K, N)) ** 3, rng.gamma(1.0, 1.0, size=K * (K - 1) // 2)


def _close(a, b):
    return abs(a - b) <= RTOL * max(abs(a), abs(b))


@pytest.mark.parametrize("K,N", CASES)
def test_the_mirror_equals_brute_force(K, N):
    rng = np.random.default_rng(100 * K + N)
    worst = 0.0
    for _ in range(3):
        g, Phi = _case(rng, K, N)
        Z, S, R = J.recursion(K, N, g, Phi)
        Zb, Sb, Rb = J.brute_force(K, N, g, Phi)
        pairs = [(Z, Zb)] + [(S[k][l], Sb[k][l]) for k in range(K) for l in range(N)] + list(zip(R, Rb))
        worst = max(worst, max(abs(a - b) / max(abs(a), abs(b)) for a, b in pairs))
        assert all(_close(a, b) for a, b in pairs)
    print("K, N =", K, N, "largest relative difference", worst)


@pytest.mark.parametrize("K,N", CASES)
def test_every_dataset_s_marginals_sum_to_Z(K, N):
    rng = np.random.default_rng(200 * K + N)
    g, Phi = _case(rng, K, N)
    Z, S, _ = J.recursion(K, N, g, Phi)
    for k in range(K):
        total = 0.0
        for v in S[k]:
            total += v
        assert _close(total, Z), k


@pytest.mark.parametrize("K,N", [(2, 3), (3, 4), (4, 5)])
def test_without_Phi_the_joint_is_the_product_of_the_proposals(K, N):
    rng = np.random.default_rng(300 * K + N)
    lp = rng.normal(size=(K, N)) * 3.0
    Pi = rng.gamma(1.0, 1.0, size=(K, N))
    Pi /= Pi.sum(axis=1, keepdims=True)
    Phi = np.zeros(K * (K - 1) // 2)
    g, mx = J.weights(lp, Pi)
    Z, S, R = J.recursion(K, N, g, Phi)
    qj, fq = J.quantise(Z, S, R)
    w = []
    for k in range(K):
        q, _ = X.proposal(lp[k], Pi[k])
        F = 0.0
        for v in g[k]:
            F += v
        w.append([v / F for v in g[k]])
        assert all(_close(S[k][l] / Z, w[k][l]) for l in range(N))
        assert all(abs(a - b) <= 1 for a, b in zip(qj[k], q))
    for i, (a, b) in enumerate(J.pairs(K)):
        assert _close(R[i] / Z, sum(x * y for x, y in zip(w[a], w[b])))


def test_a_clear_dataset_lends_its_label_to_an_uninformative_one():
    """Dataset 0 has every flag off (lp = 0: g = Pi), dataset 1 is clear about label 2, Phi_01 = 50."""
    N = 4
    Pi = np.array([[0.4, 0.3, 0.2, 0.1], [0.25, 0.25, 0.25, 0.25]])
    lp = np.array([[0.0] * N, [-30.0, -30.0, 0.0, -30.0]])
    g, _ = J.weights(lp, Pi)
    Z, S, R = J.recursion(2, N, g, [50.0])
    joint0 = [v / Z for v in S[0]]
    alone0, _ = X.proposal(lp[0], Pi[0])
    assert int(np.argmax(joint0)) == 2 and int(np.argmax(alone0)) == 0
    Zb, Sb, _ = J.brute_force(2, N, g, [50.0])
    assert all(_close(a, b) for a, b in zip(S[0], Sb[0]))


def test_fused_rises_with_Phi():
    rng = np.random.default_rng(5)
    g, _ = _case(rng, 3, 4)
    last = -1.0
    for phi in (0.0, 0.5, 2.0, 10.0, 50.0):
        Z, _, R = J.recursion(3, 4, g, [phi, 0.3, 0.3])
        assert R[0] / Z > last
        last = R[0] / Z
    assert last <= 1.0 + RTOL


def test_zero_or_infinite_Z_gives_no_weight():
    assert J.quantise(0.0, [[0.0, 0.0]], [0.0]) == ([[0, 0]], [0])
    assert J.quantise(float("inf"), [[1.0, 2.0]], [1.0]) == ([[0, 0]], [0])
    assert J.quantise(float("nan"), [[1.0, 2.0]], [1.0]) == ([[0, 0]], [0])
    assert J.quantise(2.0, [[1.0, 0.5]], [2.0]) == ([[J.Q_ONE // 2, J.Q_ONE // 4]], [J.Q_ONE])


def test_the_mirror_of_the_sums_counts_labels_pairs_and_rows():
    rng = np.random.default_rng(6)
    C_, K, m, N, n = 2, 3, 4, 3, 7
    qj = rng.integers(0, J.Q_ONE, size=(C_, K, m, N))
    fq = rng.integers(0, J.Q_ONE, size=(C_, 3, m))
    incj = rng.normal(size=(C_, m))
    s = rng.integers(0, N, size=(C_, K, n)).astype(np.int32)
    s[1, 2, 3] = N                                                 # belongs to no cluster
    empty = np.zeros((C_, K, N), dtype=bool)
    empty[0, 1, 2] = True
    mir = J.Mirror(K, m, n)
    mir.add(qj, fq, incj, s, empty)
    assert int(mir.sim_joint[0, 1, 5]) == sum(int(qj[c, 0, 1, s[c, 0, 5]]) for c in range(C_))
    assert int(mir.sim_joint[2, 0, 3]) == int(qj[0, 2, 0, s[0, 2, 3]])
    assert (mir.new_cluster_joint[1] == qj[0, 1, :, 2]).all() and not mir.new_cluster_joint[[0, 2]].any()
    assert (mir.fused_new == fq.sum(axis=0)).all()
    assert (mir.lpd_joint_sum == (0.0 + incj[0]) + incj[1]).all()
    twice = J.Mirror(K, m, n)
    twice.merge(mir)
    twice.merge(mir)
    assert twice.T == 2 and (twice.fused_new == 2 * mir.fused_new).all()


def test_header_exports_and_library_agree(pkg):
    hdr = open(os.path.join(ROOT, "include", "pmdi_hip.h")).read()
    for name in NEW:
        assert re.search(rf"\bint\s+{name}\s*\(", hdr), name
        assert name in pkg.EXPORTS and hasattr(pkg.lib(), name), name
    assert pkg.lib().pmdi_abi_version() == pkg.ABI_VERSION == 2
    assert "Deliberately not computed" not in hdr
    blob = open(pkg.LIB_PATH, "rb").read()
    for kernel in (b"predict_chain_tables_kernel", b"predict_couple_kernel", b"predict_coupled_reduce_kernel", b"predict_coupled_merge_kernel"):
        assert kernel in blob, kernel
    assert issubclass(pkg.CoupledPredictiveCounts, pkg.PredictiveCounts)


def test_argument_errors_come_before_any_device_use(pkg):
    L = pkg.lib()
    out = C.c_void_p()
    assert L.pmdi_predict_create_coupled(None, 1, None, 0, C.byref(out)) == -1      # PMDI_E_ARG, like pmdi_predict_create
    assert L.pmdi_predict_add_arrays_coupled(None, None, None, None, None, None) == -1
    assert L.pmdi_predict_get_coupled(None, None, None, None, None, None) == -1
    assert L.pmdi_predict_merge_coupled(None, *[None] * 7, 0, None) == -1
    assert L.pmdi_predict_last_coupled(None, *[None] * 7) == -1
    rng = np.random.default_rng(7)
    data = [rng.normal(size=(30, 3)), rng.poisson(2.0, size=(30, 2))]
    kinds = ["GaussianCluster", "NegBinomCluster"]
    new = [rng.normal(size=(4, 3)), rng.poisson(2.0, size=(4, 2))]
    with pytest.raises(ValueError, match="predict_coupled needs predict"):      # (a PmdiError would mean the device was asked first)
        pkg.pmdi_pooled(data, kinds, 4, 8, 0.25, 3, n_chains=2, predict_coupled=True)
    with pytest.raises(ValueError, match="two or more datasets"):
        pkg.pmdi_pooled(data[:1], kinds[:1], 4, 8, 0.25, 3, n_chains=2, predict=new[:1], predict_coupled=True)
    with pytest.raises(ValueError, match="same number"):
        pkg.pmdi_pooled(data, kinds, 4, 8, 0.25, 3, n_chains=2, predict=[new[0], new[1][:3]], predict_coupled=True)


def test_coupled_counts_on_hand_made_arrays(pkg):
    T, C_, K, m, n = 2, 3, 3, 2, 4
    one = T * C_ * J.Q_ONE
    sim = np.zeros((K, m, n), dtype=np.int64)
    sim[:, :, 0] = one                                             # uncoupled: both rows with observation 0
    simj = np.zeros((K, m, n), dtype=np.int64)
    simj[:, 0, 0] = one
    simj[:, 1, 3] = one                                            # coupled: row 1 with observation 3
    fused = np.arange(3 * m, dtype=np.int64).reshape(3, m) * (one // 8)
    pc = pkg.CoupledPredictiveCounts(T, C_, sim, np.zeros((K, m)), np.zeros((K, m)), simj, np.full((K, m), one // 4), fused,
                                     np.array([-6.0, -12.0]))
    assert pc.G == 3 and pc.pairs == [(0, 1), (0, 2), (1, 2)]
    assert pc.joint_similarity().shape == (K, m, n) and pc.joint_similarity(1).shape == (m, n) and pc.joint_similarity(0)[1, 3] == 1.0
    assert (pc.joint_new_cluster() == 0.25).all() and pc.fused().shape == (3, m) and pc.fused()[2, 1] == 5 / 8
    assert pc.joint_log_predictive().tolist() == [-1.0, -2.0]
    labels = np.array([7, 7, 9, 9])
    assert pc.allocate(labels)[0].tolist() == [7, 7] and pc.allocate(labels, joint=True)[0].tolist() == [7, 9]
    assert pc.allocate(labels, k=2, joint=True)[0].tolist() == [7, 9]
    plain = pkg.PredictiveCounts(T, C_, sim, np.zeros((K, m)), np.zeros((K, m)))
    with pytest.raises(ValueError):
        plain.allocate(labels, joint=True)


def test_coupled_kernels_use_no_scratch():
    """hipcc cross-compiles without a GPU: every kernel of pmdi_predict_coupled.hip reports ScratchSize 0 and no spills (the subset
    tables are indexed by run-time masks and live in LDS)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "particlemdi.jl_amd", "csrc", "pmdi_predict_coupled.hip")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC",
                            "--cuda-device-only", "-c", src, "-o", os.path.join(tmp, "x.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    cur, scratch, vspill, sspill = None, {}, {}, {}
    for line in r.stderr.splitlines():
        for pattern, into in ((r"ScratchSize \[bytes/lane\]: (\d+)", scratch), (r"VGPRs Spill: (\d+)", vspill), (r"SGPRs Spill: (\d+)", sspill)):
            m = re.search(pattern, line)
            if m and cur:
                into[cur] = int(m.group(1))
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
    for want in ("predict_chain_tables_kernel", "predict_couple_kernel", "predict_coupled_reduce_kernel", "predict_coupled_merge_kernel"):
        assert any(want in k for k in scratch), (want, sorted(scratch))
    for k in scratch:
        assert scratch[k] == 0 and vspill[k] == 0 and sspill[k] == 0, (k, scratch[k], vspill[k], sspill[k])
