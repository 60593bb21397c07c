"""The resampling event of the settled-chain kernel on the device, on the cases of tests/test_emu_resample.py whose events need
several rounds of column and id ranks, keep ids and columns in the chain's arena and move pool rows of all three widths: the same
oracle sweeps (computed once, shared with the emulator's tests), replayed through Sweeper(..., tuning={"settled": 2}) with the default
LDS tables and with the tiny ones (2 columns, 8 ids: everything in the arena)."""
import numpy as np
import pytest

from _cases import chain_result, check_state_against_oracle, check_sweep_against_oracle
from test_emu_resample import N1, T, _reference

pytestmark = pytest.mark.gpu

TABLES = {"default": {}, "arena": {"s2_cols": 2, "s2_idcap": 8}}


@pytest.mark.parametrize("tables", list(TABLES))
@pytest.mark.parametrize("name", ["K2-P512", "K3-P1024", "gau+cat+nb-P256"])
def test_resampling_events_equal_oracle(pkg, name, tables):
    ref = _reference(name)
    if name != "gau+cat+nb-P256":
        assert (ref.ev_cols > T).any() and (ref.ev_maxid > T).any(), (ref.ev_cols.max(), ref.ev_maxid.max())
    assert (ref.moved > 0).all(), ref.moved
    sw = pkg.Sweeper(ref.data, ref.kinds, ref.N, ref.P, n_chains=1, seed=ref.seed, tuning=dict({"settled": 2, "sticky": 0, "ksplit": 0}, **TABLES[tables]))
    assert sw.settled
    if tables == "arena":
        assert (sw.layout()["s2"]["cols_l"], sw.layout()["s2"]["idcap"]) == (2, 8), sw.layout()
    all_int = all(k != "gaussian" for k in ref.kinds)
    for w in ref.sweeps:
        rg = sw.sweep(w["it"], w["s"][None], w["order"][None], N1, w["Pi"][None], w["Phi"][None], trace=True)
        wk, kern = sw.work_counters(), sw.swept_by()
        assert int(kern[0]) in (1, 2), kern
        check_sweep_against_oracle(chain_result(rg, 0), w["ro"], wk[0], (w["up"], w["mv"]), w["rec"], ref.N, int(kern[0]), all_int=all_int,
                                   where=f"{name} [{tables}] iteration {w['it']} (kernel {kern[0]})")
        check_state_against_oracle(sw.export_state(0), w["state"], ref.N, ref.P, ref.K, ref.n)
    sw.close()
