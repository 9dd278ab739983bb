"""The session's stream contract under a stalled stream: every scenario of tests/stream_cases.py runs twice on fresh sessions of the tiny
fixtures -- calm, with a synchronisation after every step, and stalled, with api.stream_delay queued in front of every library call and one
synchronisation at the end -- and every output of every step must be bit-identical between the two (stream_cases.check_exact).  Steps
declared asynchronous must return while the stream is still busy; steps declared waiting must hand back complete host results.  What each
scenario holds, and which wait of the session code it guards: DESIGN.md, "Stream contract"."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import stream_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def calm_runs(api, golden_dir):
    """The calm run of a scenario, computed once and left unchanged (the graph test compares against the same ones)."""
    cache = {}

    def get(sid):
        if sid not in cache:
            cache[sid] = sc.execute(api, golden_dir, sid, False)[0]
        return cache[sid]
    return get


@pytest.mark.parametrize("sid", sorted(sc.SCENARIOS))
def test_a_stalled_chain_gives_the_bits_of_a_calm_one(api, golden_dir, calm_runs, sid):
    calm = calm_runs(sid)
    stalled, busy = sc.execute(api, golden_dir, sid, True)
    bad = sc.compare(calm, stalled, sid)
    assert not bad, "\n".join(bad)
    declared = {k for k, (kind, _) in sc.STEPS[sc.table_id(sid)].items() if kind == sc.ASYNC}
    assert set(busy) == declared, (sorted(busy), sorted(declared))
    assert not sc.not_busy(busy), "declared asynchronous, but the stream had drained on return: %s" % sc.not_busy(busy)


def test_two_sessions_on_two_streams_do_not_wait_for_each_other(api, golden_dir):
    """Scenario H."""
    bad, busy = sc.run_H(api, golden_dir)
    assert not bad, "\n".join(bad)
    assert not sc.not_busy(busy), sc.not_busy(busy)


def test_a_returned_bank_is_complete_for_a_session_on_another_stream(api, golden_dir):
    """Scenario K."""
    bad, busy = sc.run_K(api, golden_dir)
    assert not bad, "\n".join(bad)
    assert not sc.not_busy(busy), sc.not_busy(busy)


def test_stalled_chains_with_graphs_enabled(golden_dir, calm_runs):
    """Scenario J: chains A to C in a fresh child process with DINOV2_HIP_GRAPHS=1 (read once per process), each chain repeated on one
    session until its forwards are replayed from captured graphs; the bits equal this process's calm runs without graphs."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import sys; sys.path.insert(0, 'tests'); import stream_cases as sc; sc.child_main(sys.argv[1], sys.argv[2])"
    with tempfile.TemporaryDirectory() as td:
        f = os.path.join(td, "graphs.npz")
        out = subprocess.run([sys.executable, "-c", code, golden_dir, f], cwd=root, env=dict(os.environ, DINOV2_HIP_GRAPHS="1"),
                             capture_output=True, text=True, timeout=300)
        assert "STREAMS_OK" in out.stdout, out.stdout + out.stderr
        got = dict(np.load(f))
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("NOT_BUSY")]
    assert [ln[1] for ln in lines] == list(sc.GRAPH_SCENARIOS) and all(ln[2] == "-" for ln in lines), out.stdout
    bad = []
    for sid in sc.GRAPH_SCENARIOS:
        bad += sc.compare(calm_runs(sid), {k.split("/", 1)[1]: v for k, v in got.items() if k.startswith(sid + "/")}, sid + " with graphs")
    assert not bad, "\n".join(bad)
