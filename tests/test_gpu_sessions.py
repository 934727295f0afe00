"""Vehicle sessions on the GPU (DESIGN.md §3 rule 12; sessions.hip) against the sequential model of
tests/stream_ref.py over the oracle: windows, forwarded reports, final store and histogram must be
the model's bit for bit, however the arrivals are cut into pushes.

Inputs (checked on the CPU with the model alone): conftest's small_world, 32 vehicles x 400 points
at 1 Hz.  Set A, the stock thresholds: 274 triggers, 183 trims, 91 whole-list clears, 13 forwarded;
set B (1200 m / 20 / 150 s): 88 triggers, 80 forwarded.  No evaluated distance comes closer than
0.03 m to its threshold (Java's Math.cos is not det_cos; a stated deviation)."""
import ctypes

import numpy as np
import pytest

import stream_ref as sr
from reporter_amd import _lib, engine, graphfile, world

pytestmark = pytest.mark.gpu

B_PARAMS = dict(dist=1200.0, count=20, time_s=150.0)
GRANS = {"per_point": 0, "20s": 20.0, "150s": 150.0, "one_push": None}


def _model(g, arr, n_vehicles, opts=None, **kw):
    m = sr.Sessions(n_vehicles, sr.oracle_matcher(g, engine.default_options(1) if opts is None else opts), **kw)
    m.push(arr["vehicle"], arr["time"], arr["lon"], arr["lat"], arr["accuracy"], arr["stamp_ms"])
    return m


@pytest.fixture(scope="module")
def ctx(built_lib, small_world):
    g = graphfile.load(small_world)
    tr = world.generate_traces(small_world, n_traces=32, n_points=400, rate_s=1.0, noise_m=5.0, seed=11)
    arr = sr.interleave(tr)
    eng = engine.Engine(small_world, 0)
    bm = engine.BatchMatcher(eng)
    c = {"g": g, "tr": tr, "arr": arr, "eng": eng, "bm": bm, "path": small_world,
         "A": _model(g, arr, 32), "B": _model(g, arr, 32, **B_PARAMS)}
    yield c
    bm.close()
    eng.close()


class Hist:
    def __init__(self, nseg):
        self.nseg = nseg
        self.h, self.d = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(_lib.lib().rm_device_alloc(nseg * 64, ctypes.byref(self.h)))
        _lib.check(_lib.lib().rm_device_alloc(nseg * 8, ctypes.byref(self.d)))
        _lib.check(_lib.lib().rm_device_memset(self.h, 0, nseg * 64))
        _lib.check(_lib.lib().rm_device_memset(self.d, 0, nseg * 8))

    def get(self):
        hist, dur = np.empty(self.nseg * 16, np.uint32), np.empty(self.nseg, np.uint64)
        _lib.check(_lib.lib().rm_device_download(hist.ctypes.data, self.h, hist.nbytes))
        _lib.check(_lib.lib().rm_device_download(dur.ctypes.data, self.d, dur.nbytes))
        return hist, dur

    def free(self):
        _lib.lib().rm_device_free(self.h)
        _lib.lib().rm_device_free(self.d)


class Collected:
    """The calls' outputs concatenated: arrival made global (push start + index), window made an
    index into the concatenated windows."""

    def __init__(self):
        self.windows, self.reports, self.counts, self.max_rounds = [], [], {}, 0
        self.n_win = 0

    def add(self, sess, out, start=None):
        w, r = sess.windows().copy(), sess.reports().copy()
        assert len(r) == out["forwarded"]
        if start is not None:
            w["arrival"] += np.uint32(start)
        r["window"] += np.uint32(self.n_win)
        self.n_win += len(w)
        self.windows.append(w)
        self.reports.append(r)
        for k, v in out.items():
            if k != "rounds":
                self.counts[k] = self.counts.get(k, 0) + v
        self.max_rounds = max(self.max_rounds, out["rounds"])

    def cat(self):
        return np.concatenate(self.windows), np.concatenate(self.reports)


def _push_all(sess, arr, cuts):
    col = Collected()
    for a, b in cuts:
        out = sess.push(arr["vehicle"][a:b], arr["time"][a:b], arr["lon"][a:b], arr["lat"][a:b], arr["accuracy"][a:b],
                        arr["stamp_ms"][a:b])
        col.add(sess, out, a)
    return col


def _same_store(got, want):
    for k in ("cnt", "max_sep", "last_update", "lon", "lat", "time", "accuracy"):
        assert got[k].tobytes() == want[k].tobytes(), k


def _same(col, model, store=None):
    w, r = col.cat()
    mw, mr = model.window_array(), model.report_array()
    assert w.tobytes() == mw.tobytes(), (len(w), len(mw))
    assert r.tobytes() == mr.tobytes(), (len(r), len(mr))
    for k, v in model.counts.items():
        assert col.counts[k] == v, (k, col.counts, model.counts)
    if store is not None:
        _same_store(store, model.store())


def _session_kw(kw):
    return dict(report_dist_m=kw.get("dist"), report_count=kw.get("count"), report_time_s=kw.get("time_s"),
                max_vehicle_points=kw.get("max_points", 0))


def test_inputs_are_not_vacuous(ctx):
    a, b = ctx["A"], ctx["B"]
    assert a.counts["triggers"] >= 200 and a.counts["cleared"] >= 50 and a.counts["trims"] >= 100, a.counts
    assert b.counts["forwarded"] >= 60, b.counts
    assert a.closest > 1e-3 and b.closest > 1e-3, (a.closest, b.closest)
    assert a.counts["failed"] == 0 and b.counts["failed"] == 0


@pytest.mark.parametrize("gran", list(GRANS))
def test_granularity_parity_and_histogram_a(ctx, gran):
    """Set A at one granularity: windows, reports, store and the accumulated histogram / duration
    sums equal the model's, hence each other's across the four granularities."""
    model = ctx["A"]
    h = Hist(ctx["eng"].n_segments)
    try:
        sess = engine.VehicleSessions(ctx["bm"], 32, hist_dev=h.h.value, dur_dev=h.d.value)
        col = _push_all(sess, ctx["arr"], sr.slices(ctx["arr"], GRANS[gran]))
        _same(col, model, sess.store())
        if gran == "one_push":
            assert col.max_rounds >= 3, col.max_rounds
        hist, dur = h.get()
        want_h, want_d = model.histogram(ctx["eng"].n_segments)
        np.testing.assert_array_equal(hist, want_h)
        np.testing.assert_array_equal(dur, want_d)
        assert int(hist.sum()) > 0
        print("sessions A", gran, col.counts, "rounds", col.max_rounds, sess.ms())
        sess.close()
    finally:
        h.free()


@pytest.mark.parametrize("gran", ["150s", "one_push"])
def test_parameter_set_b(ctx, gran):
    model = ctx["B"]
    sess = engine.VehicleSessions(ctx["bm"], 32, **_session_kw(B_PARAMS))
    col = _push_all(sess, ctx["arr"], sr.slices(ctx["arr"], GRANS[gran]))
    _same(col, model, sess.store())
    assert col.counts["forwarded"] >= 60
    sess.close()


def _one_trace(tr, k, n):
    o = int(tr["trace_off"][k])
    return {f: np.asarray(tr[f][o:o + n]) for f in ("time", "lon", "lat", "accuracy")}


@pytest.mark.parametrize("n_arr", [15, 16, 17, 63, 64, 65])
def test_group_step_edges(ctx, n_arr):
    """One vehicle takes n_arr arrivals in one push: the trigger on the last arrival, then on the
    first arrival of a 16-arrival step (list index 1, 17 or 49).  Beside it a vehicle with no new
    points, the last vehicle index, a push in which nothing triggers and an empty push."""
    g, tr, NV = ctx["g"], ctx["tr"], 7
    first_of_step = 1 if n_arr < 18 else (17 if n_arr < 50 else 49)
    for count in (n_arr, first_of_step + 1):
        kw = dict(dist=0.0, count=count, time_s=0.0)
        model = sr.Sessions(NV, sr.oracle_matcher(g, engine.default_options(1)), **kw)
        sess = engine.VehicleSessions(ctx["bm"], NV, **_session_kw(kw))
        col = Collected()
        # nothing triggers: one point for vehicle 3, one for the last vehicle
        p = {f: np.concatenate([_one_trace(tr, 3, 1)[f], _one_trace(tr, 6, 1)[f]]) for f in ("time", "lon", "lat", "accuracy")}
        veh = np.array([3, NV - 1], np.uint32)
        out = sess.push(veh, p["time"], p["lon"], p["lat"], p["accuracy"], 7)
        assert out["triggers"] == 0 and out["rounds"] == 0 and out["arrivals"] == 0
        col.add(sess, out, 0)
        model.push(veh, p["time"], p["lon"], p["lat"], p["accuracy"], 7)
        out = sess.push(np.zeros(0, np.uint32), np.zeros(0), np.zeros(0, np.float32), np.zeros(0, np.float32))
        assert out == dict.fromkeys(engine.SESSION_COUNTS, 0)
        col.add(sess, out, 0)
        # vehicle 0: n_arr arrivals; the last vehicle: 3 more, interleaved at the front
        a, z = _one_trace(tr, 0, n_arr), _one_trace(tr, 6, 4)
        veh = np.concatenate([[0, NV - 1, 0, NV - 1, NV - 1], np.zeros(n_arr - 2, np.uint32)]).astype(np.uint32)
        idx0, idxz = np.nonzero(veh == 0)[0], np.nonzero(veh == NV - 1)[0]
        p = {}
        for f in ("time", "lon", "lat", "accuracy"):
            p[f] = np.zeros(len(veh), a[f].dtype)
            p[f][idx0] = a[f]
            p[f][idxz] = z[f][1:]
        out = sess.push(veh, p["time"], p["lon"], p["lat"], p["accuracy"], 9)
        col.add(sess, out, 0)
        model.push(veh, p["time"], p["lon"], p["lat"], p["accuracy"], 9)
        assert model.counts["triggers"] >= 1
        _same(col, model, sess.store())
        st = sess.store()
        assert st["cnt"][3] == 1 and st["last_update"][3] == 7
        sess.close()


def test_max_vehicle_points(ctx):
    tr, NV = ctx["tr"], 3
    kw = dict(dist=1e9, max_points=20)
    model = sr.Sessions(NV, sr.oracle_matcher(ctx["g"], engine.default_options(1)), **kw)
    sess = engine.VehicleSessions(ctx["bm"], NV, **_session_kw(kw))
    a = _one_trace(tr, 1, 70)
    veh = np.full(70, 2, np.uint32)
    col = Collected()
    col.add(sess, sess.push(veh, a["time"], a["lon"], a["lat"], a["accuracy"], 3), 0)
    model.push(veh, a["time"], a["lon"], a["lat"], a["accuracy"], 3)
    _same(col, model, sess.store())
    w, _ = col.cat()
    assert len(w) == 3 and all(w["err"] == engine.SESSION_CAPPED) and sess.store()["cnt"][2] == 10
    sess.close()


def test_punctuate(ctx):
    """After set A, half the vehicles are stale (their arrivals carry older stamps): they report
    with (0, 2, 0) and are gone, the others are untouched; a second punctuate evicts the rest; a
    vehicle with one point is dropped silently."""
    g, arr, NV = ctx["g"], dict(ctx["arr"]), 33
    arr["stamp_ms"] = arr["stamp_ms"] + np.where(arr["vehicle"] >= 16, 100000, 0)
    t_end = int(arr["time"].max() * 1000)
    for f, v in (("vehicle", 32), ("time", arr["time"][-1]), ("lon", arr["lon"][-1]), ("lat", arr["lat"][-1]),
                 ("accuracy", -1.0), ("stamp_ms", t_end)):
        arr[f] = np.concatenate([arr[f], np.array([v], arr[f].dtype)])
    model = _model(g, arr, NV)
    sess = engine.VehicleSessions(ctx["bm"], NV)
    col = _push_all(sess, arr, sr.slices(arr, None))
    before = sess.store()
    _same(col, model, before)
    assert before["cnt"][32] == 1 and (before["cnt"][:32] >= 2).sum() >= 24
    for ts, gone in ((t_end + 60001, range(0, 16)), (t_end + 400000, range(0, 33))):
        out = sess.punctuate(ts)
        model.punctuate(ts)
        col.add(sess, out)
        st = sess.store()
        _same(col, model, st)
        assert all(st["cnt"][v] == 0 for v in gone)
        if ts == t_end + 60001:
            assert st["cnt"][32] == 0 and np.array_equal(st["cnt"][16:32], before["cnt"][16:32])
            assert out["triggers"] >= 8 and out["rounds"] == 1
    assert sess.store()["cnt"].sum() == 0
    out = sess.punctuate(t_end + 500000)
    assert out["triggers"] == 0 and len(sess.windows()) == 0
    sess.close()


def test_bad_input_leaves_the_session_as_it_was(ctx):
    sess = engine.VehicleSessions(ctx["bm"], 4)
    a = _one_trace(ctx["tr"], 2, 5)
    sess.push(np.full(5, 1, np.uint32), a["time"], a["lon"], a["lat"], a["accuracy"], 11)
    before = sess.store()
    with pytest.raises(RuntimeError, match="vehicle index out of range"):
        sess.push(np.array([1, 4], np.uint32), a["time"][:2], a["lon"][:2], a["lat"][:2], a["accuracy"][:2], 12)
    t = a["time"][:2].copy()
    t[1] = np.nan
    with pytest.raises(RuntimeError, match="NaN"):
        sess.push(np.array([1, 2], np.uint32), t, a["lon"][:2], a["lat"][:2], a["accuracy"][:2], 12)
    _same_store(sess.store(), before)
    sess.close()


def _row_drive(g, rank_lo, rank_hi, by, along, n=118, speed=10.0, t0=2000.0):
    """n points at 1 Hz along the grid nodes whose `by` coordinate ranks in [rank_lo, rank_hi),
    ordered by `along`, at `speed` m/s from node to node."""
    lon, lat = np.asarray(g["node_lon"], np.float64), np.asarray(g["node_lat"], np.float64)
    c = {"lon": lon, "lat": lat}
    row = np.argsort(c[by], kind="stable")[rank_lo:rank_hi]
    row = row[np.argsort(c[along][row], kind="stable")]
    x, y = lon[row], lat[row]
    seg = np.hypot(np.diff(x) * 111320.0 * np.cos(np.radians(y[0])), np.diff(y) * 110567.0)
    cum = np.concatenate([[0.0], np.cumsum(seg)])
    s = np.minimum(np.arange(n) * speed, cum[-1] - 1.0)
    return {"time": t0 + np.arange(n, dtype=np.float64), "lon": np.interp(s, cum, x).astype(np.float32),
            "lat": np.interp(s, cum, y).astype(np.float32), "accuracy": np.full(n, -1.0, np.float32)}


def test_failure_isolation(built_lib, tmpdir_session):
    """Dense 60x60 @ 20 m world, one 120 m search radius for all: a vehicle in the middle of the
    grid has more than 192 roads inside its radius and its window fails with the per-trace
    candidate error (a data error the engine records); it is cleared alone and counted, while the
    vehicles along the rim of the same push keep the model's exact results."""
    path = str(tmpdir_session / "sess_dense.rmg")
    world.build_world(path, 60, 60, 20.0, seed=2, cell_m=20.0)
    g = graphfile.load(path)
    opts = engine.default_options(1, search_radius=120.0)
    drives = [_row_drive(g, 0, 60, "lat", "lon"), _row_drive(g, 30 * 60, 31 * 60, "lat", "lon"),
              _row_drive(g, 0, 60, "lon", "lat")]
    bad = 1
    n = len(drives[0]["time"])
    tr = {f: np.concatenate([d[f] for d in drives]) for f in drives[0]}
    tr["trace_off"] = np.arange(4, dtype=np.uint32) * n
    eng = engine.Engine(path, 0)
    bm = engine.BatchMatcher(eng)
    try:
        # the premise, through the plain batch path: only the middle vehicle's trace fails
        bm.set_isolation(True)
        bm.run(tr["trace_off"], tr["lon"], tr["lat"], tr["time"], tr["accuracy"], opts)
        errs = bm.trace_errors()
        assert errs[bad] & 1 and errs[0] == 0 and errs[2] == 0, errs
        bm.set_isolation(False)
        arr = sr.interleave(tr)
        oracle = sr.oracle_matcher(g, opts)
        fn = lambda v, lon, lat, t, acc: (1, -1, np.zeros(0, engine.REPORT_DTYPE)) if v == bad else oracle(v, lon, lat, t, acc)
        model = sr.Sessions(3, fn)
        model.push(arr["vehicle"], arr["time"], arr["lon"], arr["lat"], arr["accuracy"], arr["stamp_ms"])
        assert model.counts["failed"] >= 1 and model.counts["triggers"] > model.counts["failed"]
        sess = engine.VehicleSessions(bm, 3, opts=opts)
        col = _push_all(sess, arr, sr.slices(arr, None))
        _same(col, model, sess.store())
        assert col.counts["failed"] == model.counts["failed"]
        w, _ = col.cat()
        assert all(w["err"][w["vehicle"] == bad] == 1) and all(w["err"][w["vehicle"] != bad] == 0)
        sess.close()
    finally:
        bm.close()
        eng.close()
