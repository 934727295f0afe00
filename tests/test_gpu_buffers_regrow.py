"""The device buffers, part timers and scan / sort scratch the stream stages share (dev_util.hpp),
on the paths that small fixtures do not reach: a call of nothing, a first call of 3 items and then
one of about 5,000 on the same object (past the 4,096-item minimum capacities and the 1,024-window
floor, so every buffer and the hipcub scratch regrow between the calls), rows that must survive a
store's growth, and HBM given back: 50 objects of each kind created and destroyed, and 50
constructors that throw, leave the free bytes as they were.

Each second result is compared with the reference its own test file uses: the sequential models of
tests/anonymiser_ref.py, tests/stream_ref.py and tests/messages_ref.py, the oracle with the tile
restatement (test_gpu_stages.py) and the matched-edges restatement (tests/matched_edges_ref.py).
Empty pushes, adds, flushes and parses are also covered where those files test their stage.

The matcher and the engine own their blocks the same way, so the same is asked of them: a
BatchMatcher that regrows through run() and through rm_match_batch's device JSON path, matchers and
engines created and destroyed, and a workspace growth that fails, each against the oracle and
hipMemGetInfo."""
import ctypes
import json
import time

import numpy as np
import pytest

import anonymiser_ref as ar
import matched_edges_ref as me
import meili_oracle as mo
import messages_ref
import msg_text
import stream_ref as sr
from parity_util import check_reports, compare_all
from reporter_amd import _lib, engine, graphfile, world
from test_gpu_json_device import _compact
from test_gpu_matched_edges import assert_edges_equal
from test_gpu_sessions import _push_all, _same
from test_gpu_stages import _oracle, _oracle_tiles, _stream
from test_gpu_tilestore import _add, _flush, _simple

pytestmark = pytest.mark.gpu

B_PARAMS = dict(dist=1200.0, count=20, time_s=150.0)
SMALL, LARGE = 3, 5000


@pytest.fixture(scope="module")
def ctx(built_lib, small_world):
    g = graphfile.load(small_world)
    tr = world.generate_traces(small_world, n_traces=32, n_points=400, rate_s=1.0, noise_m=5.0, seed=11)
    arr = {k: v[:SMALL + LARGE] for k, v in sr.interleave(tr).items()}
    eng = engine.Engine(small_world, 0)
    bm = engine.BatchMatcher(eng)
    yield {"g": g, "arr": arr, "eng": eng, "bm": bm, "path": small_world}
    bm.close()
    eng.close()


def test_tile_store_regrows_and_keeps_its_rows():
    store, model = engine.TileStore(0, 3600, 2, "smpl_rprt", "auto", initial_rows=64), ar.Anonymiser(3600, 2)
    assert store.add(*[np.zeros(0, dt) for dt in (np.uint64, np.uint64, np.float64, np.float64, np.int32, np.int32)]) == \
        dict.fromkeys(engine.TILE_ADD_COUNTS, 0)
    assert store.flush() == ({}, dict.fromkeys(engine.TILE_FLUSH_COUNTS, 0))
    segs = _simple(2 * SMALL + LARGE, [8, 16, 9], 21)
    _add(store, model, segs[:SMALL])
    _, counts = _flush(store, model)             # flush buffers and scratch sized for 3 rows
    assert counts["rows_in"] == SMALL
    _add(store, model, segs[SMALL:2 * SMALL])    # these rows are held while the store grows past 64 rows
    held = _add(store, model, segs[2 * SMALL:])["held"]
    assert held >= SMALL + LARGE
    files, counts = _flush(store, model)         # the model holds the early rows: so must the files
    assert counts["rows_in"] == held and 0 < counts["rows_kept"] <= held and len(files) >= 4
    store.close()


def test_session_regrows(ctx):
    arr = ctx["arr"]
    model = sr.Sessions(32, sr.oracle_matcher(ctx["g"], engine.default_options(1)), **B_PARAMS)
    model.push(arr["vehicle"], arr["time"], arr["lon"], arr["lat"], arr["accuracy"], arr["stamp_ms"])
    assert model.counts["triggers"] >= 10 and model.counts["forwarded"] >= 3, model.counts
    sess = engine.VehicleSessions(ctx["bm"], 32, report_dist_m=1200.0, report_count=20, report_time_s=150.0)
    col = _push_all(sess, arr, [(0, 0), (0, SMALL), (SMALL, SMALL + LARGE)])
    _same(col, model, sess.store())
    sess.close()


def test_directory_regrows(ctx):
    """3 names, then 5,000 points of 5,000 vehicles: the call's group buffers, the arena and the scan
    scratch regrow; three of the names are known by then."""
    arr = dict(ctx["arr"])
    arr["vehicle"] = np.concatenate([np.arange(SMALL), np.arange(LARGE)]).astype(np.uint32)
    fmt = msg_text.formats(engine)[0]
    model = messages_ref.Directory(8192)
    sess = engine.VehicleSessions(ctx["bm"], 8192)
    vdir = engine.VehicleDirectory(8192)
    out, info = sess.push_messages([b""], fmt, vdir)
    assert out["arrivals"] == 0 and vdir.size == 0 and vdir.names() == []
    for a, b in ((0, SMALL), (SMALL, SMALL + LARGE)):
        chunk = msg_text.text(arr, 0, a, b)
        sess.push_messages([chunk], fmt, vdir)
        want = model.assign(messages_ref.parse([chunk], fmt)["point_names"])
        assert ctx["bm"].line_points()["uuid"].tobytes() == np.asarray(want, np.uint32).tobytes()
    assert vdir.size == LARGE and vdir.names() == model.names()
    vdir.close()
    sess.close()


def test_points_tiles_and_matched_edges_regrow(ctx):
    g, bm = ctx["g"], ctx["bm"]
    pts = _stream(ctx["path"], n_veh=11)
    assert len(pts["uuid"]) >= LARGE
    first = np.flatnonzero(pts["uuid"] == 0)
    first = first[np.argsort(pts["time"][first], kind="stable")][:SMALL]   # one window of 3 points
    none = {k: v[:0] for k, v in pts.items()}
    bm.run_points(none["uuid"], none["time"], none["lon"], none["lat"], none["accuracy"], inactivity=120, n_uuids=1)
    assert bm.sizes()["traces"] == 0 and len(bm.matched_edges()[1]) == 0
    for sel, n_wins in ((first, 1), (slice(None), 22)):
        p = {k: v[sel] for k, v in pts.items()}
        bm.run_points(p["uuid"], p["time"], p["lon"], p["lat"], p["accuracy"], inactivity=120)
        wins, tr, ref = _oracle(g, p)
        assert len(wins) == n_wins
        np.testing.assert_array_equal(bm.trace_uuid(), np.array([u for u, _ in wins], np.uint32))
        assert_edges_equal(bm.matched_edges(), me.matched_edges(g, tr, ref)[:4], "%d windows" % n_wins)
        compare_all(bm, ref, tr["trace_off"])
        for privacy in (1, 2):
            assert bm.tiles(privacy=privacy) == _oracle_tiles(ref, tr, privacy)
    assert len(bm.tiles(privacy=1)) >= 4


def _free_bytes():
    """hipMemGetInfo's free bytes, asked of the HIP runtime the library has loaded."""
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = ctypes.CDLL(path)
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipDeviceSynchronize() == 0 and hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def _objects(ctx):
    """One of each kind, megabytes each: a block left behind shows in the free bytes."""
    return [lambda: engine.TileStore(0, 3600, 2, "smpl_rprt", "auto"), lambda: engine.VehicleSessions(ctx["bm"], 1 << 16),
            lambda: engine.VehicleDirectory(1 << 16)]


def test_teardown_gives_hbm_back(ctx):
    for make in _objects(ctx):
        make().close()             # (what the first object of a kind loads stays loaded)
        before = _free_bytes()
        alive = make()
        assert _free_bytes() < before   # the figure sees one object's buffers
        alive.close()
        for _ in range(50):
            make().close()
        after = _free_bytes()
        print("free bytes before / after 50 objects:", before, after)
        assert after == before


def test_failed_constructors_give_hbm_back(ctx):
    bad = [lambda: engine.TileStore(0, 3600, 0, "smpl_rprt", "auto"), lambda: engine.VehicleSessions(ctx["bm"], 0),
           lambda: engine.VehicleDirectory(0)]
    for make in _objects(ctx):
        make().close()
    before = _free_bytes()
    for make in bad:
        for _ in range(50):
            with pytest.raises(_lib.RmError):
                make()
    after = _free_bytes()
    print("free bytes before / after 150 failed constructors:", before, after)
    assert after == before


# ---- the matcher and the engine (engine.hip's Workspace, Matcher and Engine; capi.cpp's staging) ----

def _run(bm, tr, **kw):
    return bm.run(tr["trace_off"], tr["lon"], tr["lat"], tr["time"], tr["accuracy"], **kw)


def _match(g, tr, opts=None):
    T = len(tr["trace_off"]) - 1
    return mo.match(g, mo.Batch(tr["trace_off"], tr["lon"], tr["lat"], tr["time"], tr["accuracy"],
                                engine.default_options(1) if opts is None else opts, np.zeros(T, np.uint32)))


@pytest.fixture(scope="module")
def batches(ctx):
    """The batches of these tests and the oracle's results, computed once and left unchanged: 3
    points, 5,000 (40 x 125), and test_workspace_exact_size_fallback's 1,250 and 1,750."""
    gen = lambda n, pts, seed: world.generate_traces(ctx["path"], n_traces=n, n_points=pts, rate_s=1.0, noise_m=5.0, seed=seed)
    b = {"tiny": gen(1, SMALL, 31), "large": gen(40, 125, 32), "fits": gen(10, 125, 79), "too_big": gen(14, 125, 80)}
    assert [int(b[k]["trace_off"][-1]) for k in ("tiny", "large", "fits", "too_big")] == [SMALL, LARGE, 1250, 1750]
    b["ref"] = {k: _match(ctx["g"], b[k]) for k in ("tiny", "large", "fits")}
    return b


@pytest.mark.parametrize("small_batch_points", [None, "0"], ids=["one_upload", "seven_copies"])
def test_matcher_regrows_through_run(ctx, batches, monkeypatch, small_batch_points):
    """No traces, 3 points, then 5,000 on one matcher: past the first workspace's 3 + 64 points and
    1 + 16 traces, so every group of the workspace, the pools, the small run's staging block and
    the download buffers regrow.  RM_SMALL_BATCH_POINTS=0 sends the same through the ordinary
    run's seven uploads."""
    if small_batch_points is not None:
        monkeypatch.setenv("RM_SMALL_BATCH_POINTS", small_batch_points)
    bm = engine.BatchMatcher(ctx["eng"])
    none = {"trace_off": np.zeros(1, np.uint32), "lon": np.zeros(0, np.float32), "lat": np.zeros(0, np.float32),
            "time": np.zeros(0, np.float64), "accuracy": np.zeros(0, np.float32)}
    _run(bm, none)
    assert bm.sizes()["traces"] == 0
    for name in ("tiny", "large"):
        tr, ref = batches[name], batches["ref"][name]
        t0 = time.perf_counter()
        _run(bm, tr)
        print("run of %d points after the one before: %.2f ms" % (int(tr["trace_off"][-1]), 1e3 * (time.perf_counter() - t0)))
        c = compare_all(bm, ref, tr["trace_off"])          # segments() among them: grow_dl_dev, grow_dl_host
        n_reports = check_reports(bm, ref, tr)             # reports(): the same buffers, other records
        if name == "large":
            assert c["segments"] > 200 and n_reports > 0, (c, n_reports)
    bm.close()


def _short_requests(path, n):
    """n compact requests of 2 and 3 points in turn."""
    tr = world.generate_traces(path, n_traces=n, n_points=3, rate_s=1.0, noise_m=5.0, seed=33)
    keep = np.concatenate([np.arange(3 * k, 3 * k + 2 + k % 2) for k in range(n)])
    cut = {k: tr[k][keep] for k in ("lon", "lat", "time", "accuracy")}
    cut["trace_off"] = np.concatenate([[0], np.cumsum([2 + k % 2 for k in range(n)])]).astype(np.uint32)
    return [_compact(cut, k) for k in range(n)]


def test_device_json_path_regrows(ctx, tmp_path, monkeypatch):
    """rm_match_batch's device JSON path (forced as test_gpu_json_device.py forces it; the library
    keeps no counter of it): 2 requests, then 1,100 on the same matcher, past json_reserve's
    1,024-trace floor, so the per-trace span, flag and time arrays regrow.  Every reply equals the
    one a fresh matcher gives the same call alone, and the one the host parser gives; eight of the
    requests are also sent alone, each to a fresh matcher of its own (1,100 fresh matchers would
    take the better part of a minute)."""
    import valhalla
    monkeypatch.setenv("RM_JSON_DEVICE_MIN_MB", "0")
    reqs = _short_requests(ctx["path"], 1100)
    valhalla.Configure(valhalla.write_config(str(tmp_path / "nc.json"), ctx["path"], device=0, coalesce=False))

    def alone(rs):
        sm = valhalla.SegmentMatcher()
        try:
            return sm.MatchMany(rs)
        finally:
            sm.close()

    sm = valhalla.SegmentMatcher()
    first, second = sm.MatchMany(reqs[:2]), sm.MatchMany(reqs)
    sm.close()
    assert first == alone(reqs[:2]) and second[:2] == first
    assert second == alone(reqs)
    for k in (0, 1, 2, 511, 1023, 1024, 1025, 1099):
        assert alone([reqs[k]]) == [second[k]], k
    monkeypatch.setenv("RM_JSON_DEVICE_MIN_MB", "100000")   # the host parser
    assert alone(reqs) == second
    assert sum(len(json.loads(r)["segments"]) for r in second) > 100


def test_matcher_teardown_gives_hbm_back(ctx, batches):
    """A matcher that grew its workspace, pools, staging and download buffers leaves nothing behind
    (the first ten are a warm-up: the HIP runtime may keep memory per stream)."""
    def once():
        bm = engine.BatchMatcher(ctx["eng"])
        _run(bm, batches["large"])
        assert len(bm.segments()[1]) > 200
        bm.close()

    for _ in range(10):
        once()
    before = _free_bytes()
    for _ in range(40):
        once()
    after = _free_bytes()
    print("free bytes after 10 / 50 matchers:", before, after)
    assert after == before


def test_engine_teardown_gives_hbm_back(ctx, batches):
    """An engine that built its route balls and turn rows gives the graph and both back."""
    turns = engine.default_options(1, turn_penalty_factor=200.0)

    def once():
        eng = engine.Engine(ctx["path"], 0)
        bm = engine.BatchMatcher(eng)
        _run(bm, batches["tiny"])
        assert eng.ball_stats(0)["keys"] > 0 and not eng.turn_rows()
        _run(bm, batches["tiny"], opts=turns)
        assert eng.turn_rows()
        bm.close()
        eng.close()

    for _ in range(3):
        once()
    before = _free_bytes()
    for _ in range(7):
        once()
    after = _free_bytes()
    print("free bytes after 3 / 10 engines:", before, after)
    assert after == before


def test_failed_grow_leaves_free_bytes(ctx, batches, monkeypatch):
    """A workspace that cannot grow (RM_TEST_WS_POINTS_LIMIT, as test_workspace_exact_size_fallback)
    is released whole, twenty times over, and the matcher then runs a batch that fits: a second
    round of the same calls ends with the free bytes of the first."""
    bm = engine.BatchMatcher(ctx["eng"])
    free = []
    for _ in range(2):
        monkeypatch.setenv("RM_TEST_WS_POINTS_LIMIT", "1400")
        for _ in range(20):
            with pytest.raises(RuntimeError, match="does not fit in HBM"):
                _run(bm, batches["too_big"])
        monkeypatch.delenv("RM_TEST_WS_POINTS_LIMIT")
        _run(bm, batches["fits"])
        free.append(_free_bytes())
    print("free bytes after each round of 20 failed grows and a run:", free)
    assert free[1] == free[0]
    compare_all(bm, batches["ref"]["fits"], batches["fits"]["trace_off"])
    bm.close()
