"""The launch planner (csrc/pmdi_plan.cpp) without a GPU: tests/plan_main.cpp, a program of its own built with
-fsanitize=address,undefined (nothing sanitized is loaded into Python), replays the plans recorded on the MI355X at the parent of
the commit that introduced the planner (tests/golden/sweep_plans.npz, written by tests/golden/make_sweep_plans.py): the return
code, all 32 words of the layout and the LDS bytes must be equal.  A recorded case is replayed when the workgroups of its split
form, ceil(n_chains / 8) 8 K, are no more than the recorded CU count: then any occupancy >= 1 gives the same answer, and the
callback returns 1.  Only the cases with 300 and 3 072 chains are beyond that; tests/test_gpu_plan_golden.py replays those too."""
import functools
import os
import subprocess

import numpy as np
import pytest

import _plan_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "particlemdi.jl_amd", "csrc")


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "plan_main")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",       # the runtimes are part of the program: nothing is preloaded
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC,
           os.path.join(ROOT, "tests", "plan_main.cpp"), os.path.join(CSRC, "pmdi_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(rows, cus, wait_value, occupancy=1):
        """Per row of `rows` (case tables as tests/_plan_cases.py encodes them): rc, 32 words, LDS bytes, times the occupancy
        callback was asked, error text."""
        text = "".join(" ".join(str(int(v)) for v in row) + f" {cus} {wait_value} {occupancy}\n" for row in rows)
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
        out = []
        for line in r.stdout.splitlines():
            nums, msg = line.split("|", 1)
            v = [int(x) for x in nums.split()]
            out.append(dict(rc=v[0], words=v[1:33], lds=v[33], asked=v[34], msg=msg))
        assert len(out) == len(rows)
        return out
    return run


@functools.lru_cache(maxsize=None)
def _golden():
    return PC.load()


def test_recorded_plans_replay_on_the_host(planner):
    z = _golden()
    cus, wait_value = (int(v) for v in z["device"])
    cases = [PC.decode(r) for r in z["cases"]]
    keep = [i for i, c in enumerate(cases) if PC.split_grid(c) <= cus]
    left_out = [i for i in range(len(cases)) if i not in keep]
    assert all(cases[i]["n_chains"] in (300, 3072) for i in left_out)
    assert len(left_out) <= sum(c["n_chains"] in (300, 3072) for c in cases) and len(keep) >= 300
    got = planner(z["cases"][keep], cus, wait_value)
    refused = 0
    for i, g in zip(keep, got):
        where = f"case {i}: {cases[i]}"
        assert g["rc"] == int(z["rc"][i]), where
        assert g["words"] == z["layout"][i].tolist(), where
        assert g["lds"] == int(z["lds_bytes"][i]), where
        if g["rc"]:
            refused += 1
            assert "bytes of LDS (> 160 KiB)" in g["msg"], (where, g["msg"])
        else:
            assert g["msg"] == "", (where, g["msg"])
    assert refused >= 3          # the shapes recorded because their creation fails


K2 = dict(K=2, N=6, P=256, D=4, settled=0)          # (without the settled-chain kernel the split form is the default for K > 1)


def test_split_form_that_is_not_resident_falls_back_to_one_workgroup(planner):
    """4 CUs, one workgroup each: the 16 workgroups of eight chains' split form are not resident at once.  Left alone the plan is,
    word for word, the single-workgroup form's; the occupancy callback is asked exactly once, and never without the split form."""
    auto, off = planner([PC.case(**K2, n_chains=8), PC.case(**K2, n_chains=8, ksplit=0)], 4, 1)
    assert auto["rc"] == off["rc"] == 0 and auto["words"] == off["words"] and auto["lds"] == off["lds"]
    assert auto["words"][17] == 0 and (auto["asked"], off["asked"]) == (1, 0)
    resident, = planner([PC.case(**K2, n_chains=8)], 16, 1)
    assert resident["words"][17] == 1 and resident["words"][18] == 0 and resident["lds"] < auto["lds"]


def test_forced_split_form_goes_out_in_residency_sized_batches(planner):
    forced, = planner([PC.case(**K2, n_chains=8, ksplit=1)], 4, 1)
    assert forced["rc"] == 0 and forced["words"][17] == 1 and forced["words"][18] == 8          # never fewer than eight slots
    forced, = planner([PC.case(**K2, n_chains=300, ksplit=1)], 64, 1)
    assert forced["rc"] == 0 and forced["words"][17] == 1 and forced["words"][18] == (64 // 16) * 8 == 32
    forced, = planner([PC.case(**K2, n_chains=300, ksplit=1)], 64, 0)                            # (an occupancy below 1 counts as 1)
    assert forced["words"][18] == 32
