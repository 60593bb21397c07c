"""pmdi_create decides for every recorded configuration what it decided at the commit the record was taken at
(tests/golden/sweep_plans.npz, tests/golden/make_sweep_plans.py): the return code of creation, all 32 words of
pmdi_sweep_layout and pmdi_lds_bytes.  Creation only, on the tiny data of tests/_plan_cases.py -- no sweep.  This is the only place
where the cases beyond the residency limit (300 and 3 072 chains: the occupancy the device reports decides) are replayed;
tests/test_plan_host.py replays the others through the host planner."""
import numpy as np
import pytest

import _plan_cases as PC

pytestmark = pytest.mark.gpu


def test_every_recorded_plan_is_what_pmdi_create_decides(pkg):
    import torch
    z = PC.load()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus == int(z["device"][0]), f"recorded on a device with {int(z['device'][0])} CUs, this one has {cus}"
    wrong = []
    for i, row in enumerate(z["cases"]):
        c = PC.decode(row)
        rc, words, lds = PC.create(pkg, c)
        if rc != int(z["rc"][i]) or not np.array_equal(words, z["layout"][i]) or lds != int(z["lds_bytes"][i]):
            wrong.append((i, c, rc, int(z["rc"][i]), words.tolist(), z["layout"][i].tolist(), lds, int(z["lds_bytes"][i])))
    assert not wrong, (len(wrong), wrong[:3])
