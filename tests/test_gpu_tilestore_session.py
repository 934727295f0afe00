"""A tile store fed device-to-device from vehicle sessions (DESIGN.md §3 rules 12 and 13):
after every push and after a final punctuate the session's forwarded reports join the store
straight from its device buffer, and the flush must be the anonymiser model's
(tests/anonymiser_ref.py) fed the session model's (tests/stream_ref.py) forwarded reports in
order, byte for byte.

Inputs (checked on the CPU with the two models alone): conftest's small_world, the traces and the
set-B thresholds of test_gpu_sessions.py (32 vehicles x 400 points at 1 Hz; 1200 m / 20 / 150 s):
80 reports forwarded by the pushes and 8 more by the final punctuate, 88 in all.  At quantisation
60 they make 178 rows in 34 tiles.  Privacy 1 keeps all 178 in 34 files (17,002 blob bytes);
privacy 2 -- the smallest at which the model both keeps and culls -- keeps 81 rows in 26 files and
culls 97 (privacy 3: 15 rows in 5 files; privacy 4: nothing)."""
import numpy as np
import pytest

import anonymiser_ref as ar
import stream_ref as sr
from reporter_amd import _lib, engine, graphfile, world

pytestmark = pytest.mark.gpu

B_PARAMS = dict(dist=1200.0, count=20, time_s=150.0)
Q = 60


@pytest.fixture(scope="module")
def ctx(built_lib, small_world):
    g = graphfile.load(small_world)
    tr = world.generate_traces(small_world, n_traces=32, n_points=400, rate_s=1.0, noise_m=5.0, seed=11)
    arr = sr.interleave(tr)
    ts = int(arr["time"].max() * 1000) + 10 ** 7
    model = sr.Sessions(32, sr.oracle_matcher(g, engine.default_options(1)), **B_PARAMS)
    model.push(arr["vehicle"], arr["time"], arr["lon"], arr["lat"], arr["accuracy"], arr["stamp_ms"])
    n_push = len(model.reports)
    model.punctuate(ts)
    segs = [(int(r["id"]), int(r["next_id"]), float(r["t0"]), float(r["t1"]), int(r["length"]), int(r["queue_length"]))
            for r, _, _ in model.reports]
    eng = engine.Engine(small_world, 0)
    bm = engine.BatchMatcher(eng)
    yield {"arr": arr, "ts": ts, "segs": segs, "n_push": n_push, "eng": eng, "bm": bm}
    bm.close()
    eng.close()


def _session(ctx):
    return engine.VehicleSessions(ctx["bm"], 32, report_dist_m=B_PARAMS["dist"], report_count=B_PARAMS["count"],
                                  report_time_s=B_PARAMS["time_s"])


def test_inputs_are_not_vacuous(ctx):
    assert ctx["n_push"] == 80 and len(ctx["segs"]) == 88
    kept = {}
    for privacy in (1, 2):
        m = ar.Anonymiser(Q, privacy)
        assert m.add(ctx["segs"]) == {"kept": 88, "skipped": 0, "rows": 178, "held": 178}
        kept[privacy] = m.flush()[1]
    assert kept[1] == {"rows_in": 178, "rows_kept": 178, "tiles": 34, "files": 34, "bytes": 17002}
    assert kept[2]["rows_kept"] == 81 and kept[2]["files"] == 26   # keeps some, culls some: the smallest such privacy


@pytest.mark.parametrize("privacy", [1, 2])
@pytest.mark.parametrize("gran", ["20s", "one_push"])
def test_session_to_store(ctx, gran, privacy):
    arr = ctx["arr"]
    sess = _session(ctx)
    store = engine.TileStore(0, Q, privacy, initial_rows=32)
    model = ar.Anonymiser(Q, privacy)
    want_add = model.add(ctx["segs"])
    kept = rows = 0
    for a, b in sr.slices(arr, {"20s": 20.0, "one_push": None}[gran]):
        out = sess.push(arr["vehicle"][a:b], arr["time"][a:b], arr["lon"][a:b], arr["lat"][a:b], arr["accuracy"][a:b],
                        arr["stamp_ms"][a:b])
        c = store.add_session(sess)
        assert c["kept"] == out["forwarded"] and c["skipped"] == 0
        kept += c["kept"]
        rows += c["rows"]
        assert c["held"] == rows
    assert kept == ctx["n_push"]
    out = sess.punctuate(ctx["ts"])
    c = store.add_session(sess)
    assert c["kept"] == out["forwarded"] == len(ctx["segs"]) - ctx["n_push"]
    assert (kept + c["kept"], rows + c["rows"], c["held"]) == (want_add["kept"], want_add["rows"], want_add["held"])
    files, counts = store.flush()
    mfiles, mcounts = model.flush()
    assert list(files.items()) == list(mfiles.items())
    assert counts == mcounts
    print("tile store from sessions", gran, privacy, counts, store.ms())
    assert store.flush()[0] == {}
    store.close()
    sess.close()


def test_closed_or_foreign_session_fails_cleanly(ctx):
    store = engine.TileStore(0, Q, 1)
    sess = _session(ctx)
    sess.close()
    with pytest.raises(_lib.RmError, match="session is NULL"):
        store.add_session(sess)
    n = engine.C.c_int(0)
    _lib.check(_lib.lib().rm_device_count(engine.C.byref(n)))
    if n.value >= 2:   # a store on another GPU than the session's
        other = engine.TileStore(1, Q, 1)
        live = _session(ctx)
        with pytest.raises(_lib.RmError, match="another device"):
            other.add_session(live)
        live.close()
        other.close()
    store.add(np.array([9], np.uint64), np.array([ar.INVALID_SEGMENT_ID], np.uint64), np.array([10.0]), np.array([20.0]),
              np.array([1], np.int32), np.array([0], np.int32))
    files, counts = store.flush()
    assert counts["rows_kept"] == 1 and list(files) == ["0_59/1/1"]
    store.close()
