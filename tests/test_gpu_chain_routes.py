"""Same launches as before: every call of tests/chain_route_cases.py, under every setting of the fallback matrix (set in-process: the
switches are read per call), launches exactly the kernels - profiler label by label, launch count by launch count - that
tests/golden/chain_routes.json holds.  That file was recorded by tools/record_chain_routes.py on the commit BEFORE the launch
path was put behind one plan (chain_plan.h); it is a record of that commit, never refreshed from the code under test.  A change
that moves a route on purpose records the file anew at ITS parent and says so.

Results are compared against nothing here: parity is the other tests' job."""
import json
import os

import pytest

import chain_route_cases as crc

SELFCHECK = bool(os.environ.get("VOFOD_TEST_HARNESS_SELFCHECK"))  # oracle against oracle: no kernels
OUTSIDE = crc.outside_switches()  # (read at import: the cases set switches of their own later)


@pytest.fixture(scope="module")
def inputs():
    return crc.Inputs()


@pytest.fixture(scope="module")
def golden():
    return json.loads(crc.GOLDEN.read_text())["routes"]


def test_the_golden_file_covers_every_setting_and_call(golden):
    """(no GPU needed)"""
    calls = [name for name, _ in crc.WARM_CALLS + crc.COLD_CALLS + crc.BRICK_CALLS]
    assert sorted(golden) == sorted(crc.settings())
    for setting, routes in golden.items():
        assert sorted(routes) == sorted(calls), setting


@pytest.mark.gpu
@pytest.mark.skipif(SELFCHECK, reason="oracle against oracle: no kernels are launched")
@pytest.mark.skipif(bool(OUTSIDE), reason=f"a fallback switch set from outside moves the routes: {OUTSIDE}")
@pytest.mark.parametrize("setting", crc.settings())
def test_same_launches_as_recorded(hip, inputs, golden, setting, monkeypatch):
    for k, v in crc.setting_env(setting).items():
        monkeypatch.setenv(k, v)
    got = crc.routes_of_setting(hip, inputs)
    want = golden[setting]
    different = {call: {"recorded": want[call], "launched": got[call]} for call in want if got.get(call) != want[call]}
    assert not different, json.dumps(different, indent=1, sort_keys=True)
    assert sorted(got) == sorted(want)
