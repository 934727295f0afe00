"""Matched edges on the GPU (DESIGN.md §3 rule 10; edges.hip).

Every case compares BatchMatcher.matched_edges() with the independent restatement
(tests/matched_edges_ref.py, run on the oracle's outputs): offsets, records field by field and the
shape, floats as bits; compare_all passes afterwards (the stage leaves the run's outputs alone).
"""
import json
import math
import os

import numpy as np
import pytest

import matched_edges_ref as me
import meili_oracle as mo
from matched_points_ref import Roads
from parity_util import compare_all
from reporter_amd import engine, graphfile, world

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _oracle(g, tr, opts, topt):
    return mo.match(g, mo.Batch(tr["trace_off"], tr["lon"], tr["lat"], tr["time"], tr["accuracy"], opts, topt))


def assert_edges_equal(got, want, what=""):
    """got: BatchMatcher.matched_edges(); want: the restatement's first four outputs."""
    g_eo, g_rec, g_so, g_sh = got
    w_eo, w_rec, w_so, w_sh = want
    assert g_rec.dtype == engine.MATCHED_EDGE_DTYPE and g_sh.dtype == np.float32 and g_sh.shape[1:] == (2,), what
    np.testing.assert_array_equal(g_eo, w_eo, err_msg=what + ": edge_off")
    np.testing.assert_array_equal(g_so, w_so, err_msg=what + ": shape_off")
    assert len(g_rec) == len(w_rec) and len(g_sh) == len(w_sh), (what, len(g_rec), len(w_rec), len(g_sh), len(w_sh))
    for f in w_rec.dtype.names:
        a, b = g_rec[f], w_rec[f]
        if a.dtype.kind == "f":
            a, b = a.view(np.uint64), b.view(np.uint64)
        if not np.array_equal(a, b):
            i = int(np.nonzero(a != b)[0][0])
            raise AssertionError("%s: field %s differs at visit %d (%d visits differ): gpu %s reference %s" % (
                what, f, i, int((a != b).sum()), g_rec[i], w_rec[i]))
    a, b = g_sh.view(np.uint32), w_sh.view(np.uint32)
    if not np.array_equal(a, b):
        i = int(np.nonzero((a != b).any(axis=1))[0][0])
        raise AssertionError("%s: shape differs at vertex %d (%d differ): gpu %s reference %s" % (
            what, i, int((a != b).any(axis=1).sum()), g_sh[i], w_sh[i]))


def run_and_compare(path, tr, opts, topt=None, what=""):
    """One run of the batch, matched_edges() against the restatement; returns (got, restatement, oracle, graph)."""
    g = graphfile.load(path)
    T = len(tr["trace_off"]) - 1
    topt = np.zeros(T, np.uint32) if topt is None else topt
    ref = _oracle(g, tr, opts, topt)
    want = me.matched_edges(g, tr, ref)
    eng = engine.Engine(path, 0)
    bm = engine.BatchMatcher(eng)
    bm.run(tr["trace_off"], tr["lon"], tr["lat"], tr["time"], tr["accuracy"], opts, topt)
    got = bm.matched_edges()
    assert bm.matched_edges_ms() > 0.0
    assert_edges_equal(got, want[:4], what)
    compare_all(bm, ref, tr["trace_off"])
    bm.close()
    eng.close()
    return got, want, ref, g


def _set(path, hz4=False, seed=301):
    if hz4:
        return world.generate_traces(path, n_traces=40, n_points=120, rate_s=0.25, noise_m=5.0, seed=seed)
    return world.generate_traces(path, n_traces=40, n_points=60, rate_s=1.0, noise_m=5.0, seed=seed)


@pytest.mark.parametrize("hz4", [False, True])
def test_baseline(built_lib, small_world, hz4):
    """1. The 1 Hz and 4 Hz sets; at 4 Hz a vehicle stays on one edge across many states."""
    got, want, ref, g = run_and_compare(small_world, _set(small_world, hz4), engine.default_options(1),
                                        what="4hz" if hz4 else "1hz")
    assert len(got[1]) > (100 if hz4 else 300) and len(got[3]) > len(got[1])
    if hz4:
        assert max(b - a + 1 for a, b in want[4]) >= 5


def test_window_carry(built_lib, small_world):
    """2. 8 x 300 points at 4 Hz: traces of more than two 64-record windows, and visits whose records
    lie either side of a window boundary (the open visit carried in wave-uniform registers)."""
    tr = world.generate_traces(small_world, n_traces=8, n_points=300, rate_s=0.25, noise_m=5.0, seed=476)
    got, want, ref, g = run_and_compare(small_world, tr, engine.default_options(1), what="window carry")
    nrec = [int(ref["path_cnt"][tr["trace_off"][k]:tr["trace_off"][k + 1]].sum()) for k in range(8)]
    assert max(nrec) > 128, nrec
    assert sum(a // 64 != b // 64 for a, b in want[4]) >= 1


def test_long_paths(built_lib, tmpdir_session):
    """3. The sparse world at 120 s: paths of tens of edges read from the pool beyond the inline
    count, traces of more than 64 records, visits of one record or of the two either side of a state."""
    path = str(tmpdir_session / "me_gpu_sparse.rmg")
    world.build_world(path, 48, 48, 100.0, seed=12, cell_m=100.0)
    tr = world.generate_traces(path, n_traces=40, n_points=12, rate_s=120.0, noise_m=5.0, seed=302)
    got, want, ref, g = run_and_compare(path, tr, engine.default_options(1, search_radius=60.0), what="long paths")
    chained = (ref["chain_start"] == 0) & (ref["choice"] >= 0)
    assert (ref["path_cnt"][chained] > 16).sum() > 20
    assert sum(int(ref["path_cnt"][tr["trace_off"][k]:tr["trace_off"][k + 1]].sum()) > 64 for k in range(40)) > 20
    assert max(b - a + 1 for a, b in want[4]) <= 2


def test_osm_city_modes(built_lib, tmp_path_factory):
    """4. Curved multi-vertex ways in two modes: interior shape vertices, also against a road's direction."""
    d = tmp_path_factory.mktemp("me_city")
    city = world.build_city(str(d / "city.rmg"), rows=24, cols=24, seed=7)
    tr = world.concat_traces(world.generate_traces(city, 20, 60, rate_s=1.0, noise_m=5.0, seed=81, mode="auto"),
                             world.generate_traces(city, 20, 60, rate_s=1.0, noise_m=5.0, seed=82, mode="pedestrian"))
    opts = engine.default_options(2)
    opts[1]["mode"] = world.MODES["pedestrian"]
    got, want, ref, g = run_and_compare(city, tr, opts, np.repeat(np.arange(2, dtype=np.uint32), 20), what="city")
    rec = got[1]
    first = (rec["flags"] & me.CHAIN_FIRST) != 0
    inner = rec["shape_end"].astype(np.int64) - rec["shape_begin"] - 1 - first
    rev = (g["edges"].reshape(-1, 4)[rec["edge"].astype(np.int64), 3] & 1) != 0
    assert (inner >= 1).sum() > 50
    assert ((inner >= 2) & rev).sum() >= 3      # the descending order


def _assemble(traces):
    off = np.concatenate([[0], np.cumsum([len(t[0]) for t in traces])]).astype(np.uint32)
    out = {k: np.concatenate([np.asarray(t[i], np.float64) for t in traces]) for i, k in enumerate(("lon", "lat", "time"))}
    out["accuracy"] = np.full(int(off[-1]), 5.0, np.float32)
    out["trace_off"] = off
    return out


def test_hand_made_batch(built_lib, small_world):
    """5. A 90-point stop, a vehicle that only stands, a state 5 km off the map, a jump beyond the
    breakage distance and a two-point trace."""
    base = _set(small_world, seed=311)
    rng = np.random.default_rng(5)
    mlat, mlon = 110567.0, 111320.0 * math.cos(math.radians(float(base["lat"][0])))

    def tr(k, a=0, b=60):
        o = int(base["trace_off"][k])
        return [base[f][o + a:o + b].copy() for f in ("lon", "lat", "time")]

    def jitter(lon, lat, n, m):
        r, th = rng.uniform(0, m, n), rng.uniform(0, 2 * math.pi, n)
        return lon + r * np.cos(th) / mlon, lat + r * np.sin(th) / mlat

    traces = []
    lon, lat, t = tr(0, 0, 20)                                           # drives 20 s, stands 90 s
    jl, ja = jitter(lon[-1], lat[-1], 90, 2.9)
    traces.append((np.concatenate([lon, jl]), np.concatenate([lat, ja]), np.concatenate([t, t[-1] + 1 + np.arange(90)])))
    lon, lat, t = tr(1, 0, 1)                                            # only stands: one state, no path
    jl, ja = jitter(lon[0], lat[0], 90, 2.9)
    traces.append((np.concatenate([lon, jl]), np.concatenate([lat, ja]), np.concatenate([t, t[0] + 1 + np.arange(90)])))
    lon, lat, t = tr(2, 0, 30)                                           # the middle state 5 km north of the map
    lat = lat.copy()
    lat[14] += 5000.0 / mlat
    traces.append((lon, lat, t))
    la, aa, ta = tr(3, 0, 20)                                            # a jump of more than 2.5 km
    k2 = next(k for k in range(4, 40) if math.hypot((base["lon"][base["trace_off"][k]] - la[-1]) * mlon,
                                                    (base["lat"][base["trace_off"][k]] - aa[-1]) * mlat) > 2500.0)
    lb, ab, _ = tr(k2, 0, 20)
    traces.append((np.concatenate([la, lb]), np.concatenate([aa, ab]), ta[0] + np.arange(40, dtype=np.float64)))
    traces.append(tuple(x[:2] for x in tr(5)))                           # two points
    batch = _assemble(traces)
    got, want, ref, g = run_and_compare(small_world, batch, engine.default_options(1), what="hand-made")
    eo, rec, so, sh = got
    off = batch["trace_off"].astype(np.int64)
    assert eo[2] == eo[1] and so[2] == so[1] and int(ref["n_states"][1]) == 1     # standing only: nothing
    for k, at in ((2, 14), (3, 20)):     # chain-first flags where the oracle breaks the chain
        tv = rec[eo[k]:eo[k + 1]]
        firsts = tv[(tv["flags"] & me.CHAIN_FIRST) != 0]
        assert len(firsts) == 2 and firsts[0]["begin_point"] == 0 and firsts[1]["begin_point"] >= at, (k, firsts)
        S = int(ref["n_states"][k])
        so_k = ref["state_orig"][off[k]:off[k] + S]
        slot = off[k] + int(np.nonzero(so_k == firsts[1]["begin_point"])[0][0])
        assert ref["chain_start"][slot]
    assert eo[5] - eo[4] >= 1 and off[5] - off[4] == 2


def test_turn_costs(built_lib, small_world):
    """6. turn_penalty_factor 200: the visits follow the oracle's (changed) choices."""
    run_and_compare(small_world, _set(small_world), engine.default_options(1, turn_penalty_factor=200.0), what="turn costs")


def test_run_paths_and_rerun(built_lib, small_world, monkeypatch):
    """7. The small run, the ordinary run (RM_SMALL_BATCH_POINTS=0) and a rerun leave the same
    bytes; the stage asked twice gives the same bytes."""
    g = graphfile.load(small_world)
    tr = _set(small_world)
    opts = engine.default_options(1)
    ref = _oracle(g, tr, opts, np.zeros(40, np.uint32))
    want = me.matched_edges(g, tr, ref)[:4]
    eng = engine.Engine(small_world, 0)
    bm = engine.BatchMatcher(eng)
    got = {}
    for way in ("small", "ordinary", "rerun"):
        if way == "ordinary":
            monkeypatch.setenv("RM_SMALL_BATCH_POINTS", "0")
        else:
            monkeypatch.delenv("RM_SMALL_BATCH_POINTS", raising=False)
        if way == "rerun":
            bm.rerun()
        else:
            bm.run(tr["trace_off"], tr["lon"], tr["lat"], tr["time"], tr["accuracy"], opts)
        out = bm.matched_edges()
        assert_edges_equal(out, want, way)
        got[way] = b"".join(x.tobytes() for x in out)
        compare_all(bm, ref, tr["trace_off"])
        assert b"".join(x.tobytes() for x in bm.matched_edges()) == got[way]
    assert got["small"] == got["ordinary"] == got["rerun"]
    bm.close()
    eng.close()


def test_isolation(built_lib, tmpdir_session):
    """8. A trace that fails under isolation (more than 192 roads in its radius) has no visits and
    an empty shape; its neighbours equal the restatement of the batch without it."""
    path = str(tmpdir_session / "me_dense.rmg")
    world.build_world(path, 60, 60, 20.0, seed=2, cell_m=20.0)
    g = graphfile.load(path)
    T = 8
    tr = world.generate_traces(path, n_traces=T, n_points=40, rate_s=1.0, noise_m=3.0, seed=73)
    opts = engine.default_options(2, search_radius=30.0)
    opts[1]["search_radius"] = 200.0
    topt = np.zeros(T, np.uint32)
    topt[3] = 1
    eng = engine.Engine(path, 0)
    bm = engine.BatchMatcher(eng)
    bm.set_isolation(True)
    bm.run(tr["trace_off"], tr["lon"], tr["lat"], tr["time"], tr["accuracy"], opts, topt)
    errs = bm.trace_errors()
    assert np.nonzero(errs)[0].tolist() == [3], errs
    eo, rec, so, sh = bm.matched_edges()
    bm.close()
    eng.close()
    assert eo[4] == eo[3] and so[4] == so[3]
    o = tr["trace_off"].astype(np.int64)
    good = [k for k in range(T) if k != 3]
    sel = np.concatenate([np.arange(o[k], o[k + 1]) for k in good])
    sub = {k: tr[k][sel] for k in ("lon", "lat", "time", "accuracy")}
    sub["trace_off"] = (np.arange(len(good) + 1) * 40).astype(np.uint32)
    ref = _oracle(g, sub, opts[:1], np.zeros(len(good), np.uint32))
    want = me.matched_edges(g, sub, ref)[:4]
    assert len(want[1]) > 30
    assert_edges_equal((np.delete(eo, 4), rec, np.delete(so, 4), sh), want, "neighbours of the failed trace")


def polyline_decode(s, factor):
    """[(lat, lon)] as integers: the inverse of the encoding, written for this test."""
    vals, cur, shift = [], 0, 0
    for ch in s:
        c = ord(ch) - 63
        assert 0 <= c < 64
        cur |= (c & 0x1F) << shift
        shift += 5
        if c < 0x20:
            vals.append(~(cur >> 1) if cur & 1 else cur >> 1)
            cur, shift = 0, 0
    assert shift == 0 and len(vals) % 2 == 0
    out, lat, lon = [], 0, 0
    for i in range(0, len(vals), 2):
        lat += vals[i]
        lon += vals[i + 1]
        out.append((lat, lon))
    return out


REQUIRED = {"edge_id", "way_id", "begin_shape_index", "end_shape_index", "begin_trace_index", "end_trace_index", "length",
            "start_time", "end_time", "source_percent_along", "target_percent_along"}
OPTIONAL = {"speed", "segment_id", "internal", "discontinuity"}


def check_reply(text, plain, rec, shape, seg_id):
    """One MatchEdges reply against Match's reply for the request and the trace's records / shape."""
    assert text.startswith(plain[:-1] + ',"edges":['), text[:200]
    rep = json.loads(text)
    assert set(rep) == {"segments", "edges", "shape"} and rep["segments"] == json.loads(plain)["segments"]
    assert len(rep["edges"]) == len(rec)
    for i, (e, r) in enumerate(zip(rep["edges"], rec)):
        has_seg, first = bool(r["flags"] & me.HAS_SEGMENT), bool(r["flags"] & me.CHAIN_FIRST)
        moving = float(r["t_exit"]) > float(r["t_enter"])
        want_keys = set(REQUIRED)
        want_keys |= {"speed"} if moving else set()
        want_keys |= {"segment_id"} if has_seg else set()
        want_keys |= {"internal"} if r["flags"] & me.INTERNAL else set()
        want_keys |= {"discontinuity"} if first and i > 0 else set()
        assert set(e) == want_keys, (i, sorted(e), sorted(want_keys))
        assert e["edge_id"] == int(r["edge"]) and e["way_id"] == int(r["way"])
        assert e["begin_shape_index"] == int(r["shape_begin"]) and e["end_shape_index"] == int(r["shape_end"])
        assert e["begin_trace_index"] == int(r["begin_point"]) and e["end_trace_index"] == int(r["end_point"])
        if has_seg:
            assert e["segment_id"] == int(seg_id[r["seg_dense"]])
        km = (int(r["e_cm"]) - int(r["b_cm"])) / 1e5
        assert e["length"] == pytest.approx(km, rel=1e-6)
        assert e["start_time"] == pytest.approx(float(r["t_enter"]), rel=1e-6)
        assert e["end_time"] == pytest.approx(float(r["t_exit"]), rel=1e-6)
        assert e["source_percent_along"] == pytest.approx(int(r["b_cm"]) / int(r["len_cm"]), rel=1e-6)
        assert e["target_percent_along"] == pytest.approx(int(r["e_cm"]) / int(r["len_cm"]), rel=1e-6)
        if moving:
            assert e["speed"] == pytest.approx(km / ((float(r["t_exit"]) - float(r["t_enter"])) / 3600.0), rel=1e-6)
        for key in ("internal", "discontinuity"):
            assert e.get(key, True) is True
    def llround(x):   # half away from zero
        return int(math.copysign(math.floor(abs(x) + 0.5), x))

    want = [(llround(float(la) * 1e6), llround(float(lo) * 1e6)) for lo, la in shape]
    assert polyline_decode(rep["shape"], 1e6) == want
    return rep


def test_json_replies(built_lib, small_world, tmp_path):
    """9. MatchEdges / MatchEdgesMany: Match's text up to its closing brace, then the edges as the
    records give them and the shape at precision 6."""
    import valhalla
    g = graphfile.load(small_world)
    tr = _set(small_world)
    eng = engine.Engine(small_world, 0)
    bm = engine.BatchMatcher(eng)
    bm.run(tr["trace_off"], tr["lon"], tr["lat"], tr["time"], tr["accuracy"], engine.default_options(1))
    eo, rec, so, sh = bm.matched_edges()
    bm.close()
    eng.close()
    conf = valhalla.write_config(str(tmp_path / "me.json"), small_world, device=0)
    valhalla.Configure(conf)
    sm = valhalla.SegmentMatcher()
    reqs = [json.dumps(world.trace_to_request(tr, k), separators=(",", ":")) for k in range(4)]
    outs = [sm.MatchEdges(reqs[0])] + sm.MatchEdgesMany(reqs[1:])
    keys = set()
    for k in range(4):
        rep = check_reply(outs[k], sm.Match(reqs[k]), rec[eo[k]:eo[k + 1]], sh[so[k]:so[k + 1]], g["seg_id"])
        assert len(rep["edges"]) > 3
        for e in rep["edges"]:
            keys |= set(e)
    assert {"speed", "segment_id"} <= keys <= REQUIRED | OPTIONAL
    sm.close()


def test_manila_reply_bytes(built_lib, tmp_path):
    """9b. rm_match's reply for the README's Manila trace is what it was
    (tests/golden/manila_match_reply.json), and MatchEdges' reply starts with it."""
    import valhalla
    from test_gpu_manila import manila_world
    path = str(tmp_path / "manila.rmg")
    req = manila_world(path)
    with open(os.path.join(HERE, "golden", "manila_match_reply.json")) as f:
        want = f.read().strip()
    conf = valhalla.write_config(str(tmp_path / "manila.json"), path, device=0)
    valhalla.Configure(conf)
    sm = valhalla.SegmentMatcher()
    text = json.dumps(req, separators=(",", ":"))
    assert sm.Match(text) == want
    both = sm.MatchEdges(text)
    assert both.startswith(want[:-1] + ',"edges":[')
    rep = json.loads(both)
    assert len(rep["edges"]) >= 5 and len(polyline_decode(rep["shape"], 1e6)) == rep["edges"][-1]["end_shape_index"] + 1
    assert sm.Match(text) == want
    sm.close()
