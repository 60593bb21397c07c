"""The predictive accumulator without a GPU.  The first five tests check the YARDSTICK, tests/_np_predict.py (the CPU oracle's
clusters, Python float loops), against properties it must have: they run none of the shipped code and pass without it; what
they buy is trust in the mirror that tests/test_gpu_predict.py holds the device to.  The rest run shipped code:
PredictiveCounts.allocate on hand-made counts, the argument checks of pmdi_pooled(predict=...), which come before any device
use, and what the compiler reports for the kernels of pmdi_predict.hip."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import _np_predict as X


def _case(rng, C_=2, n=40, m=5, N=6):
    train = [rng.normal(size=(n, 3)), rng.integers(1, 5, size=(n, 4)), rng.poisson(3.0, size=(n, 2))]
    train[1][0, :] = 4
    new = [rng.normal(size=(m, 3)), rng.integers(1, 5, size=(m, 4)), rng.poisson(3.0, size=(m, 2))]
    kinds = ["gaussian", "categorical", "negbinom"]
    s = rng.integers(0, N, size=(C_, 3, n)).astype(np.int32)
    Pi = rng.gamma(1.0, 1.0, size=(C_, 3, N))
    Pi /= Pi.sum(axis=2, keepdims=True)
    return train, kinds, new, s, Pi


def test_weights_sum_to_one_in_fixed_point(O):
    rng = np.random.default_rng(1)
    train, kinds, new, s, Pi = _case(rng)
    N = Pi.shape[2]
    lp, _ = X.log_predictives(O, train, kinds, new, s, None, N)
    q, inc = X.proposals(lp, Pi)
    assert (q >= 0).all() and np.isfinite(inc).all()
    assert (np.abs(q.sum(axis=3) - X.Q_ONE) <= N / 2 + 1).all()      # N roundings of at most half a unit each, and the sum's few ulp


def test_all_flags_off_gives_the_quantised_Pi(O):
    rng = np.random.default_rng(2)
    train, kinds, new, s, Pi = _case(rng)
    C_, K, N = Pi.shape
    flags = np.zeros((C_, 9), dtype=np.uint8)
    lp, _ = X.log_predictives(O, train, kinds, new, s, flags, N)
    assert (lp == 0.0).all()
    q, inc = X.proposals(lp, Pi)
    for c in range(C_):
        for k in range(K):
            want, _ = X.proposal([0.0] * N, Pi[c, k])
            assert (q[c, k] == np.array(want)[None, :]).all()
            assert (np.abs(q[c, k, 0] - np.floor(Pi[c, k] * X.Q_ONE + 0.5)) <= 1).all()


def test_a_row_equal_to_a_tight_cluster_goes_there(O):
    rng = np.random.default_rng(3)
    n, N, D = 60, 4, 5
    centre = rng.normal(size=D)
    x = rng.normal(size=(n, D)) * 3.0
    x[:30] = centre
    s = np.concatenate([np.full(30, 2), rng.integers(0, 2, 30)]).astype(np.int32).reshape(1, 1, n)
    Pi = np.full((1, 1, N), 1.0 / N)
    lp, empty = X.log_predictives(O, [x], ["gaussian"], [centre.reshape(1, D)], s, None, N)
    q, _ = X.proposals(lp, Pi)
    assert empty[0, 0].tolist() == [False, False, False, True]
    assert q[0, 0, 0, 2] > 0.99 * X.Q_ONE


def test_sim_depends_on_an_observation_only_through_its_labels(O):
    rng = np.random.default_rng(4)
    train, kinds, new, s, Pi = _case(rng)
    s[:, :, 7] = s[:, :, 3]
    s[:, 1, 9] = s[:, 1, 3]
    N = Pi.shape[2]
    lp, empty = X.log_predictives(O, train, kinds, new, s, None, N)
    q, inc = X.proposals(lp, Pi)
    mir = X.Mirror(3, new[0].shape[0], train[0].shape[0])
    mir.add(q, inc, s, empty)
    assert (mir.sim[:, :, 7] == mir.sim[:, :, 3]).all() and (mir.sim[1, :, 9] == mir.sim[1, :, 3]).all()
    # and directly: the entry is the sum over the chains of the weight on the observation's label
    want = sum(int(q[c, 2, 1, s[c, 2, 5]]) for c in range(s.shape[0]))
    assert int(mir.sim[2, 1, 5]) == want


def test_new_cluster_is_zero_when_no_label_is_empty(O):
    rng = np.random.default_rng(5)
    train, kinds, new, s, Pi = _case(rng, N=3)
    s[:, :, :3] = np.arange(3)
    lp, empty = X.log_predictives(O, train, kinds, new, s, None, 3)
    assert not empty.any()
    q, inc = X.proposals(lp, Pi)
    mir = X.Mirror(3, new[0].shape[0], train[0].shape[0])
    mir.add(q, inc, s, empty)
    assert (mir.new_cluster == 0).all() and mir.sim.sum() > 0
    s[0, 1][s[0, 1] == 2] = 0                    # label 2 of chain 0, dataset 1 is empty now: its weight is the novelty score
    lp, empty = X.log_predictives(O, train, kinds, new, s, None, 3)
    q, inc = X.proposals(lp, Pi)
    mir.reset()
    mir.add(q, inc, s, empty)
    assert (mir.new_cluster[1] == q[0, 1, :, 2]).all() and (mir.new_cluster[[0, 2]] == 0).all()


def test_allocate_on_hand_made_counts(pkg):
    T, C_ = 2, 3
    one = T * C_ * X.Q_ONE
    labels = np.array([5, 5, 2, 9, 2, 5])                          # groups 2 (two members), 5 (three), 9 (a singleton)
    sim = np.zeros((2, 4, 6), dtype=np.int64)
    sim[0, 0] = [one, one, 0, 0, 0, one]                           # row 0: all of it on group 5
    sim[0, 1] = [0, 0, one // 2, one // 4, one // 2, 0]            # row 1: group 2 at 1/2 beats the singleton at 1/4
    sim[0, 2] = [one // 2, one // 2, one // 2, one // 2, one // 2, one // 2]      # row 2: a three-way tie: the lowest group
    sim[0, 3] = [0, 0, 0, one, 0, 0]                               # row 3: the singleton
    sim[1] = sim[0][::-1]                                          # the second dataset sees the rows in the other order
    pc = pkg.PredictiveCounts(T, C_, sim, np.zeros((2, 4), dtype=np.int64), np.zeros((2, 4)))
    assigned, scores = pc.allocate(labels, k=0)
    assert assigned.tolist() == [5, 2, 2, 9] and scores.shape == (4, 3)
    assert scores[0].tolist() == [0.0, 1.0, 0.0] and scores[1].tolist() == [0.5, 0.0, 0.25] and scores[2].tolist() == [0.5, 0.5, 0.5]
    assigned1, _ = pc.allocate(labels, k=1)
    assert assigned1.tolist() == [9, 2, 2, 5]
    both, sc = pc.allocate(labels)                                 # the mean of the two datasets
    assert np.array_equal(sc, (pc.allocate(labels, k=0)[1] + pc.allocate(labels, k=1)[1]) / 2)
    assert both.tolist() == [5, 2, 2, 5]                           # rows 0 and 3: groups 5 and 9 tie at 1/2: the lowest
    assert pc.similarity().shape == (2, 4, 6) and pc.similarity(1).shape == (4, 6) and pc.similarity(0)[0, 0] == 1.0
    assert pc.new_cluster().shape == (2, 4) and pc.log_predictive().shape == (2, 4)
    with pytest.raises(ValueError):
        pc.allocate(labels[:5])
    with pytest.raises(ValueError):
        pkg.PredictiveCounts(0, C_, sim, np.zeros((2, 4)), np.zeros((2, 4))).similarity()


def test_pooled_argument_errors_come_before_any_device_use(pkg):
    rng = np.random.default_rng(6)
    n = 30
    data = [rng.normal(size=(n, 3)), rng.integers(1, 4, size=(n, 2)), rng.poisson(2.0, size=(n, 2))]
    data[1][0, 0] = 3
    kinds = ["GaussianCluster", "CategoricalCluster", "NegBinomCluster"]
    good = [rng.normal(size=(4, 3)), rng.integers(1, 4, size=(4, 2)), rng.poisson(2.0, size=(4, 2))]

    def run(predict):
        return pkg.pmdi_pooled(data, kinds, 4, 8, 0.25, 3, n_chains=2, predict=predict)

    bad_level0, bad_levelL, bad_count = [x.copy() for x in good], [x.copy() for x in good], [x.copy() for x in good]
    bad_level0[1][2, 1] = 0
    bad_levelL[1][2, 1] = 4
    bad_count[2][0, 0] = -1
    for predict, what in ((good[:2], "3 datasets"), ([good[0][:, :2], good[1], good[2]], "D="), (bad_level0, "categorical level"),
                          (bad_levelL, "categorical level"), (bad_count, "negative count"),
                          ([good[0], good[1][:3], good[2]], "same number")):
        with pytest.raises(ValueError, match=what):       # (a PmdiError would mean the device was asked first)
            run(predict)
    with pytest.raises(TypeError):
        pkg.pmdi_pooled(data, kinds, 4, 8, 0.25, 3, n_chains=2, predicts=good)


def test_predict_kernels_use_no_scratch_and_the_gather_keeps_three_waves():
    """hipcc cross-compiles without a GPU: every kernel of pmdi_predict.hip reports ScratchSize 0 and no spills, and the gather
    kernel stays within 168 VGPRs (three waves per SIMD: its flush forms the row addresses late, see the comment there)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "particlemdi.jl_amd", "csrc", "pmdi_predict.hip")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC",
                            "--cuda-device-only", "-c", src, "-o", os.path.join(tmp, "x.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    cur, scratch, vspill, vgprs = None, {}, {}, {}
    for line in r.stderr.splitlines():
        for pattern, into in ((r"ScratchSize \[bytes/lane\]: (\d+)", scratch), (r"VGPRs Spill: (\d+)", vspill), (r" VGPRs: (\d+)", vgprs)):
            m = re.search(pattern, line)
            if m and cur:
                into[cur] = int(m.group(1))
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
    for want in ("predict_weights_kernel", "predict_normalise_kernel", "predict_gather_kernel", "predict_reduce_kernel", "predict_merge_kernel"):
        assert any(want in k for k in scratch), (want, sorted(scratch))
    for k in scratch:
        assert scratch[k] == 0 and vspill[k] == 0, (k, scratch[k], vspill[k])
    gather = [k for k in vgprs if "predict_gather_kernel" in k]
    assert len(gather) == 1 and vgprs[gather[0]] <= 168, vgprs
