"""No device: the refusals of dinov2_hip_op_stream_delay, the self-checks of the case table of tests/stream_cases.py, and the agreement of
DESIGN.md's "Stream contract" table with the waits that stand in the session code."""
import os
import re

import pytest

import stream_cases as sc

WAIT = re.compile(r"hipStreamSynchronize\(|hipDeviceSynchronize\(|hipEventSynchronize\(|hipMemcpy\(")
SESSION_FILES = ("model.cpp", "extras.cpp", "resident.cpp", "pca.cpp", "kmeans.hip")


@pytest.mark.parametrize("ms", [0, -1, 101, 1000, 2**31 - 1, -2**31])
def test_stream_delay_refuses_a_length_outside_1_to_100_ms(api, ms):
    """Refused with DINOV2_HIP_ERR_INVALID before any HIP call: on a host without a device this returns 4, not a HIP error.  The stream is
    a made-up non-null handle that a launch would fault on."""
    assert api.lib().dinov2_hip_op_stream_delay(0x1000, ms) == 4
    with pytest.raises(ValueError):
        api.stream_delay(0x1000, ms)


@pytest.mark.parametrize("ms", [1, 20, 100])
def test_stream_delay_refuses_the_null_stream(api, ms):
    assert api.lib().dinov2_hip_op_stream_delay(None, ms) == 4
    with pytest.raises(ValueError):
        api.stream_delay(None, ms)
    with pytest.raises(ValueError):
        api.stream_delay(0, ms)


def test_the_stall_is_long_enough_and_bounded():
    assert 4 * sc.MEASURED_ENQUEUE_MS <= sc.STALL_MS <= 100
    for sid in sc.SCENARIOS:  # no scenario accumulates more than about a second of stall
        assert len(sc.dry_steps(sid)) * sc.STALL_MS <= 1000, sid
    assert len(sc.GRAPH_SCENARIOS) and all(len(sc.dry_steps(s)) * sc.STALL_MS * sc.GRAPH_REPEATS <= 1000 for s in sc.GRAPH_SCENARIOS)


@pytest.mark.parametrize("sid", sorted(sc.SCENARIOS))
def test_every_step_of_a_chain_is_declared(sid):
    """A chain runs exactly the steps its table row declares (an undeclared step is a KeyError in Run.step), each once."""
    steps = sc.dry_steps(sid)
    assert len(steps) == len(set(steps)) and set(steps) == set(sc.STEPS[sc.table_id(sid)]), (steps, sorted(sc.STEPS[sc.table_id(sid)]))


def test_every_waiting_step_names_its_wait():
    assert {sc.table_id(s) for s in sc.SCENARIOS} | {"H", "K"} == set(sc.STEPS)
    for sid, steps in sc.STEPS.items():
        assert any(kind == sc.ASYNC for kind, _ in steps.values()), sid  # every scenario proves that it ran behind a stall
        for name, (kind, site) in steps.items():
            assert kind in (sc.ASYNC, sc.WAITS), (sid, name)
            assert (site in sc.WAIT_SITES) if kind == sc.WAITS else site is None, (sid, name, site)


def _waits_in_code():
    found = set()
    for f in SESSION_FILES:
        for n, line in enumerate(open(os.path.join(sc.CSRC, f)), 1):
            if WAIT.search(line.split("//")[0]):
                found.add("%s:%d" % (f, n))
    return found


def test_wait_sites_point_at_waits():
    code = _waits_in_code()
    for name, (f, line, _) in sc.WAIT_SITES.items():
        assert f is None or "%s:%d" % (f, line) in code, "WAIT_SITES[%r] = %s:%d holds no wait" % (name, f, line)


def test_design_table_has_one_row_per_wait_in_session_code():
    """DESIGN.md "Stream contract": every wait of the session code has a row (file:line), no row points at a line without one, and every
    scenario named as a guard exists."""
    text = open(os.path.join(sc.ROOT, "DESIGN.md")).read()
    m = re.search(r"^## .*Stream contract.*?$(.*?)(?=^## |\Z)", text, re.S | re.M)
    assert m, "DESIGN.md has no section 'Stream contract'"
    rows = [[c.strip() for c in ln.strip().strip("|").split("|")] for ln in m.group(1).splitlines() if re.match(r"\|\s*`?\w+\.(cpp|hip):\d+", ln)]
    cited = {r[0].strip("`") for r in rows}
    code = _waits_in_code()
    assert cited == code, "rows without a wait: %s; waits without a row: %s" % (sorted(cited - code), sorted(code - cited))
    for r in rows:
        assert len(r) == 3 and r[1] and r[2], r
        if re.match(r"[A-K]: ", r[2]):  # guarded by a scenario: it exists, and its mutant's result is recorded
            assert r[2][0] in sc.STEPS and "fails as expected" in r[2], r
        elif re.match(r"redundant with line \d+", r[2]):  # ... a wait of the same file
            assert "%s:%s" % (r[0].strip("`").split(":")[0], re.match(r"redundant with line (\d+)", r[2]).group(1)) in code, r
        else:
            assert r[2].startswith(("redundant with line ", "precedes a free: argued from the code, never mutated", "not in a scenario: ")), r
    for name, (f, line, _) in sc.WAIT_SITES.items():
        assert f is None or "%s:%d" % (f, line) in cited, name
    assert str(sc.STALL_MS) + " ms" in m.group(1) and ("%g ms" % sc.MEASURED_ENQUEUE_MS) in m.group(1)
