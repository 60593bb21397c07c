"""get_consensus_allocations (consensus_map.jl:92-105) without a GPU: the numpy restatement of the library's hclust
(tests/_np_hclust.py: nearest-neighbour chain, the tie rule of include/pmdi_hip.h) is pinned by scipy, and the library's
host-only pmdi_cutree is checked against the restatement's cut.  The device kernels are compared with the same restatement
bit for bit in tests/test_gpu_hclust.py.

Not here: the linkage kernel's device source in the lock-step workgroup emulator of tests/emu/.  The kernel is written in
plain HIP (threadIdx / __shfl_xor / __syncthreads), not against the PM2_* lane API the emulator provides, so running it there
means a second body header and an emulator driver; the GPU tests compare the real kernel with the restatement bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from scipy.cluster.hierarchy import fcluster, linkage
from scipy.spatial.distance import squareform

import _np_hclust as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (2, 3, 50, 300, 1000)
# Largest relative difference between the restatement's heights and scipy's on exactly the inputs of
# _np_hclust.uniform_matrix(n), n in SIZES, measured on the CPU: single 0.0, complete 0.0, average 0.0, ward 7.201800447219e-16.  Both sides evaluate the same
# few-flop Lance-Williams update, associated differently; 64 x the measured value (never less than 4 ulp = 2^-50) leaves room
# for another libm / numpy build, not for another algorithm.
MEASURED = {"average": 0.0, "ward": 7.201800447219e-16}
RTOL = {link: max(64.0 * v, 2.0 ** -50) for link, v in MEASURED.items()}


@pytest.mark.parametrize("link", H.LINKAGES)
@pytest.mark.parametrize("n", SIZES)
def test_restatement_equals_scipy_on_tie_free_input(n, link):
    """On tie-free input the dendrogram of a reducible linkage is unique: every cut equals scipy's as a partition, exactly;
    the heights of single and complete (which only select one of their inputs) are equal, those of average and ward agree
    within RTOL (measured: see MEASURED)."""
    m = H.uniform_matrix(n)
    merges, heights, order = H.hclust(m, link)
    Z = linkage(squareform(m, checks=False), method=link)
    for k in (2, 3, 5, 10, 25):
        if k <= n:
            assert H.same_partition(H.cutree(n, merges, heights, k=k), fcluster(Z, k, "maxclust")), (n, link, k)
    assert (np.diff(heights) >= 0).all()
    rel = float(np.max(np.abs(heights - Z[:, 2]) / Z[:, 2]))
    print(f"n={n} {link}: largest relative height difference to scipy {rel:.3e}")
    if link in ("single", "complete"):
        assert np.array_equal(heights, Z[:, 2])
    else:
        assert rel <= RTOL[link], (rel, RTOL[link])


def test_single_linkage_heights_on_a_tied_psm_equal_scipy():
    """The multiset of single-linkage heights is the minimum spanning tree's: unique even with ties."""
    d, _ = H.psm_matrix()
    _, heights, _ = H.hclust(d, "single")
    Z = linkage(squareform(d, checks=False), method="single")
    assert np.array_equal(heights, np.sort(Z[:, 2]))


@pytest.mark.parametrize("link", H.LINKAGES)
def test_order_keeps_every_cluster_contiguous(link):
    for m in (H.uniform_matrix(50), H.uniform_matrix(300), H.psm_matrix()[0]):
        n = m.shape[0]
        merges, _, order = H.hclust(m, link)
        H.assert_rows_contiguous_in_order(n, merges, order)
        # the numbering itself: -i observations, +r earlier rows, each used exactly once
        used = merges.ravel().tolist()
        assert sorted(v for v in used if v < 0) == list(range(-n, 0)) and sorted(v for v in used if v > 0) == list(range(1, n - 1))
        assert all(v < r for r, row in enumerate(merges.tolist(), start=1) for v in row)


def test_restatement_recovers_the_planted_partition_of_a_tied_psm():
    d, z = H.psm_matrix()
    for link in H.LINKAGES:
        Z = linkage(squareform(d, checks=False), method=link)
        assert H.same_partition(fcluster(Z, 4, "maxclust"), z), f"scipy does not recover the planted partition ({link})"
        merges, heights, _ = H.hclust(d, link)
        assert H.same_partition(H.cutree(d.shape[0], merges, heights, k=4), z), link


def test_new_entry_points_are_declared_and_exported(pkg):
    names = {"pmdi_psm_distance_device", "pmdi_hclust_device", "pmdi_cutree"}
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pmdi_hip.h")).read(), flags=re.S)
    assert names <= set(re.findall(r"\b(pmdi_[A-Za-z_0-9]+)\s*\(", hdr))
    assert names <= set(pkg.EXPORTS)
    for name in names:
        assert hasattr(pkg.lib(), name)
    for i, name in enumerate(("SINGLE", "AVERAGE", "COMPLETE", "WARD")):
        assert re.search(rf"PMDI_LINK_{name}\s*=\s*{i}\b", hdr)
    assert pkg.lib().pmdi_abi_version() == 2


@pytest.mark.parametrize("link", H.LINKAGES)
def test_cutree_through_the_library(pkg, link):
    """pmdi_cutree is host-only: against the restatement's cut on the restatement's dendrograms, by k and by h."""
    from particlemdi_jl_amd import psm
    for m in (H.uniform_matrix(50), H.psm_matrix(n=120)[0]):
        n = m.shape[0]
        merges, heights, order = H.hclust(m, link)
        hc = psm.HClust(merges, heights, order, link)
        for k in (1, 2, n - 1, n):
            got = psm.cutree(hc, k=k)
            assert np.array_equal(got, H.cutree(n, merges, heights, k=k)) and len(set(got.tolist())) == k
            assert got[0] == 1
            first = [int(np.argmax(got == c)) for c in range(1, k + 1)]
            assert first == sorted(first), "labels are not numbered in order of first appearance"
        uniq = np.unique(heights)
        cuts = [heights[0] / 2, heights[-1] * 2, heights[n // 2], heights[-1]]
        if len(uniq) > 1:
            cuts.append((uniq[0] + uniq[1]) / 2)
        for h in cuts:
            got = psm.cutree(hc, h=float(h))
            assert np.array_equal(got, H.cutree(n, merges, heights, h=h))
            assert len(set(got.tolist())) == n - int((heights <= h).sum())          # a height equal to h is applied (<=)
        assert len(set(psm.cutree(hc, h=float(heights[0] / 2)).tolist())) == n
        assert len(set(psm.cutree(hc, h=float(heights[-1] * 2)).tolist())) == 1
        assert np.array_equal(psm.cutree(hc, k=3, h=float(heights[-1] * 2)), H.cutree(n, merges, heights, k=3))    # k wins
        for bad in (dict(k=0), dict(k=n + 1), dict()):
            with pytest.raises(pkg.PmdiError) as e:
                psm.cutree(hc, **bad)
            assert e.value.code == -1          # PMDI_E_ARG


def test_cutree_of_one_observation_and_of_bad_merges(pkg):
    from particlemdi_jl_amd import psm
    one = psm.HClust(np.zeros((0, 2), dtype=np.int64), np.zeros(0), np.ones(1, dtype=np.int64))
    assert psm.cutree(one, k=1).tolist() == [1]
    L = pkg.lib()
    merges = np.array([-1, 5, -2, -3], dtype=np.int64)         # column-major 2 x 2: row 1 = (-1, -2), row 2 = (5, -3)
    heights, labels = np.array([0.1, 0.2]), np.zeros(3, dtype=np.int64)
    rc = L.pmdi_cutree(3, merges.ctypes.data_as(C.c_void_p), heights.ctypes.data_as(C.c_void_p), 1, float("nan"),
                       labels.ctypes.data_as(C.c_void_p))
    assert rc == -1 and b"merges" in L.pmdi_last_error()


def test_consensus_allocations_need_k_or_h_and_a_device(pkg):
    import torch
    from particlemdi_jl_amd import psm
    p = psm.PosteriorSimilarityMatrix([1.0 - H.psm_matrix(n=60)[0]], ["K1"])
    with pytest.raises(ValueError, match="either k"):
        psm.get_consensus_allocations(p)
    with pytest.raises(ValueError, match="linkage"):
        psm.hclust(np.zeros((2, 2)), linkage="centroid")
    if not torch.cuda.is_available():          # no silent CPU path
        with pytest.raises(RuntimeError, match="no MI355X"):
            psm.get_consensus_allocations(p, k=4)
        with pytest.raises(RuntimeError, match="no MI355X"):
            psm.hclust(np.zeros((3, 3)))
