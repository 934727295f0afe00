"""The vehicle directory on the GPU (DESIGN.md §3 rule 14; directory.hip) against its sequential
model, a dict (tests/messages_ref.py): the same messages cut into calls of any sizes give every
point the index of the whole stream, and names() in that order -- also when RM_LINES_HASH_BITS=4
leaves 32 ids 16 hash values, so that ids share a hash inside a call and against the table.

Inputs: conftest's small_world, the interleaved arrivals of test_gpu_sessions.py (32 vehicles x 400
points at 1 Hz, seed 11; vehicle v first appears in second v) written as text by tests/msg_text.py,
and the set-B thresholds (80 forwarded reports over the pushes)."""
import numpy as np
import pytest

import messages_ref
import msg_text
import stream_ref as sr
from reporter_amd import _lib, engine, world

pytestmark = pytest.mark.gpu

B_PARAMS = dict(report_dist_m=1200.0, report_count=20, report_time_s=150.0)


def _first_split(arr):
    """Cuts right behind every vehicle's first appearance: its second one is in another call."""
    first = sorted({int(np.flatnonzero(arr["vehicle"] == v)[0]) + 1 for v in range(32)})
    cuts = [0] + first + [len(arr["vehicle"])]
    return list(zip(cuts[:-1], cuts[1:]))


def _cuts(arr, gran):
    if gran == "first_split":
        return _first_split(arr)
    return sr.slices(arr, {"one_push": None, "20s": 20.0, "1s": 0}[gran])


@pytest.fixture(scope="module")
def ctx(built_lib, small_world):
    tr = world.generate_traces(small_world, n_traces=32, n_points=400, rate_s=1.0, noise_m=5.0, seed=11)
    arr = sr.interleave(tr)
    fmt = msg_text.formats(engine)
    whole = {}
    for kind in (0, 1):
        ref = messages_ref.parse([msg_text.text(arr, kind)], fmt[kind])
        model = messages_ref.Directory(32)
        whole[kind] = (model.assign(ref["point_names"]), model.names())
    eng = engine.Engine(small_world, 0)
    bm = engine.BatchMatcher(eng)
    yield {"arr": arr, "fmt": fmt, "whole": whole, "eng": eng, "bm": bm}
    bm.close()
    eng.close()


def _run(ctx, kind, cuts, max_vehicles=32, keep=None):
    """Push the slices; returns the points' indices, the names, the flags and the outputs."""
    sess = engine.VehicleSessions(ctx["bm"], 32, **B_PARAMS)
    vdir = engine.VehicleDirectory(max_vehicles)
    idx, on_host, wins, reps = [], [], [], []
    for a, b in cuts:
        out, info = sess.push_messages([msg_text.text(ctx["arr"], kind, a, b, keep)], ctx["fmt"][kind], vdir)
        idx.append(ctx["bm"].line_points()["uuid"])
        on_host.append(info["ids_on_host"])
        wins.append(sess.windows().copy())
        reps.append(sess.reports().copy())
    names = vdir.names()
    assert vdir.size == len(names)
    vdir.close()
    sess.close()
    return np.concatenate(idx), names, on_host, wins, reps


def test_inputs_are_not_vacuous(ctx):
    arr = ctx["arr"]
    idx, names = ctx["whole"][0]
    assert len(idx) == 12800 and names == [msg_text.name(v) for v in range(32)] == ctx["whole"][1][1]
    assert len(sr.slices(arr, 0)) > 400 and len(sr.slices(arr, 20.0)) > 20
    cuts = _first_split(arr)
    assert len(cuts) == 33 and all(len(set(arr["vehicle"][a:b].tolist())) >= 1 for a, b in cuts)
    # under 4 hash bits, ids share a hash inside one call and across calls
    h = [engine_hash(msg_text.name(v).encode()) & 15 for v in range(32)]
    assert len(set(h)) < 32 and len(set(h)) <= 16


def engine_hash(b):
    h = 0xcbf29ce484222325
    for c in b:
        h = ((h ^ c) * 0x100000001b3) & 0xffffffffffffffff
    return h


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("gran", ["one_push", "20s", "1s", "first_split"])
def test_indices_do_not_depend_on_the_cut(ctx, gran, kind):
    want_idx, want_names = ctx["whole"][kind]
    idx, names, on_host, _, reps = _run(ctx, kind, _cuts(ctx["arr"], gran))
    assert idx.tobytes() == want_idx.tobytes()
    assert names == want_names
    assert sum(on_host) == 0 and sum(len(r) for r in reps) == 80


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("gran", ["one_push", "20s", "1s", "first_split"])
def test_shared_hashes(ctx, gran, kind, monkeypatch):
    """Four hash bits: ids share a hash inside a call (its numbering goes to the host) and against
    names already in the table (the lookup probes on, the insert claims the next free slot)."""
    monkeypatch.setenv("RM_LINES_HASH_BITS", "4")
    arr = ctx["arr"]
    cuts = _cuts(arr, gran)
    want_idx, want_names = ctx["whole"][kind]
    idx, names, on_host, _, reps = _run(ctx, kind, cuts)
    assert idx.tobytes() == want_idx.tobytes()
    assert names == want_names
    assert sum(len(r) for r in reps) == 80
    # the flag is set exactly for the calls in which two ids share their four bits
    h = [engine_hash(msg_text.name(v).encode()) & 15 for v in range(32)]
    shared = [int(len({h[v] for v in set(arr["vehicle"][a:b].tolist())}) < len(set(arr["vehicle"][a:b].tolist()))) for a, b in cuts]
    assert on_host == shared
    assert sum(shared) >= {"one_push": 1, "20s": 20, "1s": 400, "first_split": 20}[gran]


def test_directory_full_leaves_everything_as_it_was(ctx):
    arr = ctx["arr"]
    n = len(arr["vehicle"])
    low = arr["vehicle"] < 16
    half = n // 2
    want = _run(ctx, 0, [(0, half), (half, n)], 16, low)
    sess = engine.VehicleSessions(ctx["bm"], 32, **B_PARAMS)
    vdir = engine.VehicleDirectory(16)
    fmt = ctx["fmt"][0]
    sess.push_messages([msg_text.text(arr, 0, 0, half, low)], fmt, vdir)
    w0, r0 = sess.windows().copy(), sess.reports().copy()
    assert vdir.size == 16
    with pytest.raises(_lib.RmError, match="directory full"):
        sess.push_messages([msg_text.text(arr, 0, half, n)], fmt, vdir)   # brings the 17th id
    assert vdir.size == 16 and vdir.names() == want[1]
    sess.push_messages([msg_text.text(arr, 0, half, n, low)], fmt, vdir)
    idx = ctx["bm"].line_points()["uuid"]
    assert idx.tobytes() == want[0][-len(idx):].tobytes() and len(idx) > 1000
    assert w0.tobytes() == want[3][0].tobytes() and r0.tobytes() == want[4][0].tobytes()
    assert sess.windows().tobytes() == want[3][1].tobytes() and sess.reports().tobytes() == want[4][1].tobytes()
    assert len(want[4][0]) + len(want[4][1]) > 20
    vdir.close()
    sess.close()


def test_directory_larger_than_the_session_fails(ctx):
    sess = engine.VehicleSessions(ctx["bm"], 32, **B_PARAMS)
    vdir = engine.VehicleDirectory(33)
    with pytest.raises(_lib.RmError, match="exceeds the session's n_vehicles"):
        sess.push_messages([msg_text.text(ctx["arr"], 0, 0, 100)], ctx["fmt"][0], vdir)
    assert vdir.size == 0
    vdir.close()
    sess.close()
