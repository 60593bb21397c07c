"""The streaming PSM accumulator without a GPU: the new entry points are declared, exported and listed; pmdi_psm_acc_create
validates before it touches a device; the retention rule of pmdi_gibbs_run equals the reference's own slicing of its CSV
rows (consensus_map.jl:33,38); pmdi_pooled checks its arguments before it builds anything."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_FUNCTIONS = ["pmdi_psm_acc_create", "pmdi_psm_acc_destroy", "pmdi_psm_acc_reset", "pmdi_psm_acc_add_samples",
                 "pmdi_psm_acc_add_gibbs", "pmdi_psm_acc_merge", "pmdi_psm_acc_samples", "pmdi_psm_acc_counts", "pmdi_gibbs_run"]


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


def test_the_kernels_are_in_the_code_object(pkg):
    blob = open(pkg.LIB_PATH, "rb").read()
    for kernel in (b"psm_acc_mfma_kernel", b"psm_acc_kernel", b"psm_acc_mirror_kernel", b"psm_acc_merge_kernel"):
        assert kernel in blob, kernel


@pytest.mark.parametrize("K, n, n_labels", [(0, 10, 4), (9, 10, 4), (2, 0, 4), (2, 65536, 4), (2, 10, 256), (2, 10, -1)])
def test_create_validates_before_any_device_use(pkg, K, n, n_labels):
    h = C.c_void_p()
    assert pkg.lib().pmdi_psm_acc_create(0, K, n, n_labels, C.byref(h)) == -1       # PMDI_E_ARG, with or without a GPU
    assert not h.value
    from particlemdi_jl_amd import psm
    with pytest.raises(pkg.PmdiError) as e:
        psm.PsmAccumulator(K, n, n_labels)
    assert e.value.code == -1


def test_create_without_a_device_is_a_device_error(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; this checks the no-device error path")
    h = C.c_void_p()
    assert pkg.lib().pmdi_psm_acc_create(0, 2, 100, 12, C.byref(h)) == -2            # PMDI_E_DEVICE: there is no CPU path
    assert not h.value
    assert pkg.lib().pmdi_psm_acc_samples(None) == 0
    assert pkg.lib().pmdi_psm_acc_destroy(None) == 0


def test_null_handles_are_argument_errors(pkg):
    L = pkg.lib()
    assert L.pmdi_psm_acc_reset(None, None) == -1
    assert L.pmdi_psm_acc_add_samples(None, None, 1, None) == -1
    assert L.pmdi_psm_acc_add_gibbs(None, None, None) == -1
    assert L.pmdi_psm_acc_merge(None, None, 0, None) == -1
    assert L.pmdi_psm_acc_counts(None, None, None, None) == -1
    assert L.pmdi_gibbs_run(None, 1, 0, 1, None, None) == -1


def test_retained_iterations_is_the_reference_slicing(pkg):
    """Rows 0..iter of the CSV (row 0 = the initial state, src/pmdi.jl:158); generate_psm(file, burnin + 1, thin) reads
    rows[(burnin + 1):end] and keeps every thin-th (consensus_map.jl:33,38)."""
    from particlemdi_jl_amd import psm
    assert pkg.retained_iterations is psm.retained_iterations
    for it in (1, 2, 3, 7, 10, 12, 30):
        for burnin in range(0, it + 1):
            for thin in (1, 2, 3, 5, it, it + 1, 3 * it):
                rows = list(range(0, it + 1))
                assert psm.retained_iterations(it, burnin, thin) == rows[burnin + 1:][::thin], (it, burnin, thin)
    assert psm.retained_iterations(12, 3, 2) == [4, 6, 8, 10, 12]
    assert psm.retained_iterations(5, 0, 1) == [1, 2, 3, 4, 5]
    assert psm.retained_iterations(5, 0, 9) == [1]
    assert psm.retained_iterations(5, 5, 1) == []
    assert psm.retained_iterations(0, 0, 1) == []
    for bad in ((-1, 0, 1), (5, -1, 1), (5, 0, 0)):
        with pytest.raises(ValueError):
            psm.retained_iterations(*bad)


def _good():
    x = np.zeros((10, 2))
    return dict(dataFiles=[x, x], dataTypes=["gaussian", "gaussian"], N=3, particles=4, rho=0.25, iter=5, n_chains=2)


@pytest.mark.parametrize("change", [
    dict(dataTypes=["gaussian"]), dict(dataFiles=[np.zeros((10, 2)), np.zeros((9, 2))]), dict(rho=0.0), dict(rho=1.0),
    dict(N=1), dict(N=11), dict(particles=1), dict(rho=0.05),
    dict(n_chains=0), dict(burnin=-1), dict(burnin=5), dict(burnin=6), dict(thin=0), dict(iter=0)])
def test_pmdi_pooled_checks_its_arguments_before_building_anything(pkg, change, monkeypatch):
    P = importlib.import_module("particlemdi_jl_amd.pmdi")

    def never(*a, **k):
        raise AssertionError("pmdi_pooled built something before it had checked its arguments")
    monkeypatch.setattr(P, "Sweeper", never)
    monkeypatch.setattr(P, "Gibbs", never)
    assert pkg.pmdi_pooled is P.pmdi_pooled
    with pytest.raises(ValueError):
        P.pmdi_pooled(**{**_good(), **change})


def test_pmdi_pooled_reaches_the_device_with_good_arguments(pkg, monkeypatch):
    """The checks above are not vacuous: the same call with nothing wrong gets as far as building the Sweeper."""
    P = importlib.import_module("particlemdi_jl_amd.pmdi")

    class Reached(Exception):
        pass

    def reached(*a, **k):
        raise Reached()
    monkeypatch.setattr(P, "Sweeper", reached)
    with pytest.raises(Reached):
        P.pmdi_pooled(**_good())
    with pytest.raises(TypeError):
        P.pmdi_pooled(**{**_good(), "dataTypes": ["gaussian", "MyCluster"]})


def test_pmdi_keeps_its_own_checks(pkg, tmp_path):
    P = importlib.import_module("particlemdi_jl_amd.pmdi")
    x = np.zeros((10, 2))
    out = str(tmp_path / "o.csv")
    good = dict(dataFiles=[x], dataTypes=["gaussian"], N=3, particles=4, rho=0.25, iter=1, outputFile=out)
    for change, msg in ((dict(dataTypes=[]), "Number of datatypes"), (dict(dataNames=["a", "b"]), "Number of data names"),
                        (dict(dataFiles=[x, np.zeros((9, 2))], dataTypes=["gaussian", "gaussian"]), "same number of observations"),
                        (dict(rho=1.5), "between 0 and 1"), (dict(N=1), "Number of clusters"), (dict(N=11), "Number of clusters"),
                        (dict(particles=1), "2 or more particles"), (dict(rho=0.05), "floor")):
        with pytest.raises(ValueError, match=msg):
            P.pmdi(**{**good, **change})
    with pytest.raises(TypeError):
        P.pmdi(**{**good, "dataTypes": ["MyCluster"]})
    assert not os.path.exists(out)
