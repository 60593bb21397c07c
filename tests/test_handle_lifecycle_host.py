"""Every Python class that owns a handle of the library, after a constructor that failed before any device use: the
half-built object holds no handle, and close() -- once, twice -- and __del__ neither call the library's destroy function nor
raise.  The invalid arguments are those of the classes' own validation tests (test_abi.py::
test_argument_validation_happens_before_device_use and the test_create_validates_before_any_device_use of
test_psm_acc_host.py, test_fusion_host.py, test_summary_host.py, test_mixing_host.py, test_agreement_host.py); Gibbs and
ClusterBatch are given a sweeper without a handle, CsvWriter K = 0 and Comm a rank outside the communicator."""
import types

import numpy as np
import pytest


def _no_sweeper():
    return types.SimpleNamespace(h=None, n=10, D=[2], kinds=[0])


CASES = {
    "Sweeper": ("pmdi_destroy", lambda pkg: (([np.zeros((10, 2))], ["gaussian"], 1, 4), {})),
    "CsvWriter": ("pmdi_csv_close", lambda pkg: (("unused.csv", 0, 10), {})),
    "Comm": ("pmdi_comm_destroy", lambda pkg: ((0, 2, 2, np.zeros(128, dtype=np.uint8)), {})),
    "Gibbs": ("pmdi_gibbs_destroy", lambda pkg: ((_no_sweeper(),), {})),
    "ClusterBatch": ("pmdi_clusters_free", lambda pkg: ((_no_sweeper(), 0, 4), {})),
    "PsmAccumulator": ("pmdi_psm_acc_destroy", lambda pkg: ((0, 10, 4), {})),
    "FusionAccumulator": ("pmdi_fusion_destroy", lambda pkg: ((1, 100, 12), {"groups": ((0, 1), (0, 1, 2))})),
    "SummaryAccumulator": ("pmdi_summary_destroy", lambda pkg: ((4, 2, 1, 100), {"sumD": 5, "trace_cap": 3})),
    "MixingAccumulator": ("pmdi_mixing_destroy", lambda pkg: ((4, 2, 6, 100), {"maxlag": 1025})),
    "AgreementAccumulator": ("pmdi_agreement_destroy", lambda pkg: ((4, 2, 6, 100), {"ref": np.full(100, 255), "trace_cap": 3})),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_a_failed_constructor_leaves_nothing_to_destroy(pkg, name, monkeypatch, tmp_path):
    destroy, make = CASES[name]
    cls = getattr(pkg, name)
    args, kwargs = make(pkg)
    called = []
    monkeypatch.setattr(pkg.lib(), destroy, lambda *a: called.append(a))
    monkeypatch.chdir(tmp_path)
    obj = cls.__new__(cls)
    with pytest.raises(pkg.PmdiError) as e:
        obj.__init__(*args, **kwargs)
    assert e.value.code == -1                      # PMDI_E_ARG, with or without a GPU
    assert obj.h is None
    obj.close()
    obj.close()
    obj.__del__()
    obj.close()
    assert called == []
    assert obj.h is None
    assert not list(tmp_path.iterdir())            # (CsvWriter: no file was opened)
