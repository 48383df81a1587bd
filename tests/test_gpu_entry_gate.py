"""Same admissions as before: every call of tests/entry_gate_cases.py, in every handle state, answers exactly the status and the
error string that tests/golden/entry_refusals.json holds.  That file was recorded by tools/record_entry_refusals.py on the commit
BEFORE the entry points' admission tests were put behind one function (api_gate.h); it is a record of that commit, never
refreshed from the code under test.  A change that moves a refusal on purpose records the file anew at ITS parent and says so."""
import json
import os
import time

import pytest

import entry_gate_cases as egc

SELFCHECK = bool(os.environ.get("VOFOD_TEST_HARNESS_SELFCHECK"))  # oracle against oracle: another library's answers


@pytest.fixture(scope="module")
def golden():
    return json.loads(egc.GOLDEN.read_text())["table"]


def test_the_golden_file_covers_every_state_and_call(golden):
    """(no GPU needed)"""
    assert sorted(golden) == sorted(egc.STATES)
    for state, rows in golden.items():
        assert sorted(rows) == sorted(name for name, _ in egc.CALLS), state


def test_the_recorded_states_refuse_what_they_stand_for(golden):
    """(no GPU needed) the record itself shows that each state was reached: a table of a handle that was idle throughout would
    hold the new code to nothing"""
    busy = {state: sorted(c for c, r in rows.items() if r[0] == egc.capi.ERR_BUSY) for state, rows in golden.items()}
    assert busy["idle"] == [] and busy["world_enabled"] == []
    assert "write_map:voxels" in busy["ticket_0_in_flight"] and "process_scan" in busy["ticket_0_in_flight"]
    assert "write_map:voxels" in busy["only_ticket_1_in_flight"] and "process_batch" not in busy["only_ticket_1_in_flight"]
    assert "set_raycast_exact" in busy["raycast_rigid_pending"] and "write_map:raycast" not in busy["raycast_rigid_pending"]
    assert "write_map:raycast" in busy["raycast_exact_pending"] and "voxels_as_pc:raycast" in busy["raycast_exact_pending"]
    assert golden["sepclusters_pending"]["map_shift"] == [egc.capi.ERR_BUSY, "map shift: a sepclusters pass is pending: finish it first"]
    assert golden["world_enabled"]["world_disable"][0] == egc.capi.OK and golden["idle"]["world_disable"][0] == egc.capi.ERR_NOT_PENDING
    # the order of an entry's tests: world_disable's own state in front of the busy test, write_map's size in front of the exact pass
    assert golden["ticket_0_in_flight"]["world_disable"][0] == egc.capi.ERR_NOT_PENDING
    assert golden["raycast_exact_pending"]["write_map:raycast_short"][0] == egc.capi.ERR_SIZE_MISMATCH
    assert golden["ticket_0_in_flight"]["range_to_points:wrong_size"][0] == egc.capi.ERR_SIZE_MISMATCH


@pytest.fixture(scope="module")
def inputs(hip):
    inp = egc.Inputs(hip)
    yield inp
    inp.close()


@pytest.mark.gpu
@pytest.mark.skipif(SELFCHECK, reason="oracle against oracle: the record is the product library's")
@pytest.mark.parametrize("state", egc.STATES)
def test_same_answers_as_recorded(hip, inputs, golden, state):
    t0 = time.perf_counter()
    got = egc.rows_of_state(hip, inputs, state)
    print(f"admission table, {state}: {len(got)} calls in {time.perf_counter() - t0:.2f} s")
    want = golden[state]
    different = {call: {"recorded": want[call], "answered": got.get(call)} for call in want if got.get(call) != want[call]}
    assert not different, json.dumps(different, indent=1, sort_keys=True)
    assert sorted(got) == sorted(want)
