"""Matched edges (DESIGN.md §3 rule 10): the restatement against the oracle (CPU), one case worked
by hand, the rule's invariants, and the C-ABI additions.

The oracle keeps only the OSMLR runs it folds its traversal list into.  Folding the restatement's
visits with the same rule (form_runs below, oracle/meili_oracle.c:637-690) must reproduce every
field of the oracle's segments, floats as bits: that pins the visits' edges, extents, times and
point indices to the oracle.
"""
import ctypes

import numpy as np
import pytest

import matched_edges_ref as me
import meili_oracle as mo
from matched_points_ref import Roads
from reporter_amd import engine, graphfile, world

F = np.float32
QUEUE_SPEED_MPS = 2.7777777777777777
INVALID_SEGMENT_ID = 0x3FFFFFFFFFFF


def _oracle(g, tr, opts, topt):
    return mo.match(g, mo.Batch(tr["trace_off"], tr["lon"], tr["lat"], tr["time"], tr["accuracy"], opts, topt))


def _sets(name, small_world, tmpdir_session):
    """(graph path, traces, options, trace_opt) of the named batch."""
    if name in ("1hz", "turn200"):
        tr = world.generate_traces(small_world, n_traces=40, n_points=60, rate_s=1.0, noise_m=5.0, seed=301)
        over = dict(turn_penalty_factor=200.0) if name == "turn200" else {}
        return small_world, tr, engine.default_options(1, **over), np.zeros(40, np.uint32)
    if name == "4hz":
        tr = world.generate_traces(small_world, n_traces=40, n_points=120, rate_s=0.25, noise_m=5.0, seed=301)
        return small_world, tr, engine.default_options(1), np.zeros(40, np.uint32)
    if name == "sparse":
        path = str(tmpdir_session / "me_sparse.rmg")
        world.build_world(path, 48, 48, 100.0, seed=12, cell_m=100.0)
        tr = world.generate_traces(path, n_traces=40, n_points=12, rate_s=120.0, noise_m=5.0, seed=302)
        return path, tr, engine.default_options(1, search_radius=60.0), np.zeros(40, np.uint32)
    assert name == "city"
    city = world.build_city(str(tmpdir_session / "me_city.rmg"), rows=24, cols=24, seed=7)
    tr = world.concat_traces(world.generate_traces(city, 20, 60, rate_s=1.0, noise_m=5.0, seed=81, mode="auto"),
                             world.generate_traces(city, 20, 60, rate_s=1.0, noise_m=5.0, seed=82, mode="pedestrian"))
    opts = engine.default_options(2)
    opts[1]["mode"] = world.MODES["pedestrian"]
    return city, tr, opts, np.repeat(np.arange(2, dtype=np.uint32), 20)


@pytest.fixture(scope="module", params=["1hz", "4hz", "sparse", "city", "turn200"])
def placed(request, small_world, tmpdir_session):
    """(name, graph, Roads, traces, oracle outputs, restatement), computed once per batch."""
    path, tr, opts, topt = _sets(request.param, small_world, tmpdir_session)
    g = graphfile.load(path)
    ref = _oracle(g, tr, opts, topt)
    R = Roads(g)
    return request.param, g, R, tr, ref, me.matched_edges(g, tr, ref, R=R)


def form_runs(g, R, visits):
    """meili_oracle.c form_runs over one chain's visits: the oracle's segment fields per run."""
    out = []
    i = 0
    while i < len(visits):
        f = visits[i]
        sd, internal = int(f["seg_dense"]), bool(f["flags"] & me.INTERNAL)
        j = i + 1
        while j < len(visits):
            p, c = visits[j - 1], visits[j]
            if int(c["seg_dense"]) != sd:
                break
            if sd == me.NONE and bool(c["flags"] & me.INTERNAL) != internal:
                break
            if p["e_cm"] != p["len_cm"] or c["b_cm"] != 0:
                break
            if sd != me.NONE and int(c["seg_off_cm"]) != int(p["seg_off_cm"]) + int(p["len_cm"]):
                break
            j += 1
        l = visits[j - 1]
        start_ok = f["b_cm"] == 0 and (sd == me.NONE or f["seg_off_cm"] == 0)
        end_ok = l["e_cm"] == l["len_cm"] and (sd == me.NONE or int(l["seg_off_cm"]) + int(l["len_cm"]) == int(g["seg_len_cm"][sd]))
        if sd != me.NONE:
            length = (int(g["seg_len_cm"][sd]) + 50) // 100 if (start_ok and end_ok) else -1
        else:
            length = (sum(int(v["e_cm"]) - int(v["b_cm"]) for v in visits[i:j]) + 50) // 100
        q = 0
        for v in reversed(visits[i:j]):
            dt = float(v["t_exit"]) - float(v["t_enter"])
            d = int(v["e_cm"]) - int(v["b_cm"])
            if dt > 0.0 and (float(d) * 0.01) / dt < QUEUE_SPEED_MPS:
                q += d
            else:
                break
        way_first = way_last = int(f["way"])
        for v in visits[i + 1:j]:
            if int(v["way"]) != way_first:
                way_last = int(v["way"])
        out.append((INVALID_SEGMENT_ID if sd == me.NONE else int(g["seg_id"][sd]),
                    float(f["t_enter"]) if start_ok else -1.0, float(l["t_exit"]) if end_ok else -1.0, length,
                    (q + 50) // 100, (1 if sd == me.NONE and internal else 0) | (2 if sd != me.NONE else 0),
                    int(f["begin_point"]), int(l["end_point"]), sd, way_first, way_last))
        i = j
    return out


def _chains(rec):
    """Index ranges of the chains of one trace's visits (a chain opens at a CHAIN_FIRST visit)."""
    first = [i for i in range(len(rec)) if rec["flags"][i] & me.CHAIN_FIRST]
    assert not len(rec) or first[0] == 0
    return list(zip(first, first[1:] + [len(rec)]))


def test_fold_equals_the_oracle(placed):
    name, g, R, tr, ref, (edge_off, rec, shape_off, shape, merged) = placed
    T = len(tr["trace_off"]) - 1
    segs, seg_off = [], [0]
    for k in range(T):
        tv = rec[edge_off[k]:edge_off[k + 1]]
        for a, b in _chains(tv):
            segs += form_runs(g, R, [tv[i] for i in range(a, b)])
        seg_off.append(len(segs))
    np.testing.assert_array_equal(np.array(seg_off, np.uint32), ref["seg_off"])
    want = ref["segs"]
    assert len(segs) == len(want) > 100
    got = np.array(segs, want.dtype)
    for f in want.dtype.names:   # floats as bits
        a, b = got[f], want[f]
        if a.dtype.kind == "f":
            a, b = a.view(np.uint64), b.view(np.uint64)
        bad = np.nonzero(a != b)[0]
        assert not len(bad), (name, f, int(bad[0]), got[bad[0]], want[bad[0]])
    if name == "4hz":
        assert max(b - a + 1 for a, b in merged) >= 5    # states passed straight through on one edge
    if name == "sparse":
        # a state every two minutes: no visit folds more than the two records either side of one state
        assert max(b - a + 1 for a, b in merged) == 2 and sum(a == b for a, b in merged) > 0.9 * len(merged)


def test_invariants(placed):
    name, g, R, tr, ref, (edge_off, rec, shape_off, shape, merged) = placed
    T = len(tr["trace_off"]) - 1
    e4 = g["edges"].reshape(-1, 4)
    assert shape_off[T] == len(shape) and edge_off[T] == len(rec)
    n_first = 0
    for k in range(T):
        o, S = int(tr["trace_off"][k]), int(ref["n_states"][k])
        tv = rec[edge_off[k]:edge_off[k + 1]]
        nv = int(shape_off[k + 1] - shape_off[k])
        # route_dist of each chain of continuing slots, in order (chains without a kept record have no visits)
        dist, cur = [], None
        for s in range(S + 1):
            if s < S and me.continues(ref, o, S, s):
                cur = (cur or 0) + int(ref["route_dist"][o + s])
            elif cur is not None:
                if cur:
                    dist.append(cur)
                cur = None
        chains = _chains(tv)
        assert [sum(int(v["e_cm"]) - int(v["b_cm"]) for v in tv[a:b]) for a, b in chains] == dist, (name, k)
        n_first += len(chains)
        for a, b in chains:
            assert tv["shape_begin"][a] == (0 if a == 0 else tv["shape_end"][a - 1] + 1)
            for i in range(a, b):
                v = tv[i]
                assert v["shape_end"] - v["shape_begin"] >= 1 and v["shape_end"] < nv
                assert bool(v["flags"] & me.CHAIN_FIRST) == (i == a)
                assert v["b_cm"] < v["e_cm"] <= v["len_cm"] == e4[v["edge"], 1] and v["t_enter"] <= v["t_exit"]
                if i == a:
                    continue
                p = tv[i - 1]
                assert v["shape_begin"] == p["shape_end"]
                rp, rv = R.e_road[p["edge"]], R.e_road[v["edge"]]
                sp = p["len_cm"] - p["e_cm"] if R.e_rev[p["edge"]] else p["e_cm"]
                sv = v["len_cm"] - v["b_cm"] if R.e_rev[v["edge"]] else v["b_cm"]
                if rp == rv and sp == sv:
                    continue             # the same place on one road
                assert p["e_cm"] == p["len_cm"] and v["b_cm"] == 0, (name, k, i)
                src = int(np.searchsorted(g["node_off"], v["edge"], side="right") - 1)
                assert int(e4[p["edge"], 0]) == src, (name, k, i)          # they meet at one node
        if len(tv):
            assert tv["shape_end"][-1] == nv - 1
        else:
            assert nv == 0
    assert n_first == int((rec["flags"] & me.CHAIN_FIRST != 0).sum()) >= T // 2


# ---- one case by hand -------------------------------------------------------------------------
HAND_OSM = """<?xml version='1.0' encoding='UTF-8'?>
<osm version="0.6" generator="hand">
 <node id="1" lat="47.0000" lon="8.0000"/>
 <node id="2" lat="47.0001" lon="8.0005"/>
 <node id="3" lat="47.0003" lon="8.0010"/>
 <node id="4" lat="47.0006" lon="8.0014"/>
 <node id="5" lat="47.0010" lon="8.0017"/>
 <node id="6" lat="47.0000" lon="7.9995"/>
 <node id="7" lat="47.0000" lon="7.9990"/>
 <way id="100"><nd ref="1"/><nd ref="2"/><nd ref="3"/><nd ref="4"/><nd ref="5"/><tag k="highway" v="residential"/></way>
 <way id="200"><nd ref="1"/><nd ref="6"/><nd ref="7"/><tag k="highway" v="residential"/></way>
</osm>
"""


def test_hand_derived_case(built_lib, tmp_path):
    """Way 100 curves north-east through five vertices A0..A4 (stored distances 0, c1, c2, c3, L1),
    way 200 runs west from A0 through M to B (0, m, L2).  A vehicle is seen at A3 (t = 100), at A1
    (t = 110) and at M (t = 130): every point lies on a stored vertex, so its candidate sits at that
    vertex's stored distance (sa = c3, c1 on way 100; m on way 200) and it drives way 100 against
    its direction, on the reverse edge er, then way 200 forwards, on e2.

    Transition 1 (A3 -> A1), path [er], D = c3 - c1: one record on er, [L1 - c3, L1 - c1], times
    100 .. 110, points 0 .. 1.  Transition 2 (A1 -> M), path [er, e2], D = c1 + m: a record on er,
    [L1 - c1, L1], from t = 110 to u = 110 + 20 * (c1 / (c1 + m)), which continues the first one
    (same edge, begins where it ended) and keeps the source state's point, 1, as its end; then a
    record on e2, [0, m], from u to 130, points 1 .. 2.  Two visits:

        er  [L1 - c3, L1]  100 .. u   points 0 .. 1  first of its chain
        e2  [0, m]         u .. 130   points 1 .. 2

    Shape: the chain's first visit begins with road_point(way 100, c3), on shape segment A2-A3 at
    t = 1, i.e. A2 + 1 * (A3 - A2) in fp32; then the stored vertices strictly inside (0, c3)
    against the road's direction, A2 and A1; then road_point(way 100, 0) = A0 (t = 0).  The second
    visit has nothing strictly inside (0, m) and ends with road_point(way 200, m) = A0 + 1 * (M - A0).
    Five vertices; visit 1 spans 0 .. 3 and visit 2 spans 3 .. 4."""
    osm = tmp_path / "hand.osm"
    osm.write_text(HAND_OSM)
    g = graphfile.load(world.import_osm(str(osm), str(tmp_path / "hand.rmg"), cell_m=50.0))
    R = Roads(g)
    nv = np.diff(g["road_vert_off"].astype(np.int64))
    r1, r2 = int(np.nonzero(nv == 5)[0][0]), int(np.nonzero(nv == 3)[0][0])
    a, b = R.voff[r1], R.voff[r2]
    assert R.vlat[a] < R.vlat[a + 4] and R.vlon[b] > R.vlon[b + 2]      # stored in the ways' directions
    c1, c3, L1, m = R.cum[a + 1], R.cum[a + 3], R.cum[a + 4], R.cum[b + 1]
    assert 0 < c1 < c3 < L1 == R.len[r1] and 0 < m < R.len[r2]
    er, e2 = R.rev[r1], R.fwd[r2]
    pts = [(R.vlon[a + 3], R.vlat[a + 3]), (R.vlon[a + 1], R.vlat[a + 1]), (R.vlon[b + 1], R.vlat[b + 1])]
    tr = {"trace_off": np.array([0, 3], np.uint32), "lon": np.array([p[0] for p in pts], np.float64),
          "lat": np.array([p[1] for p in pts], np.float64), "time": np.array([100.0, 110.0, 130.0]),
          "accuracy": np.full(3, 5.0, np.float32)}
    ref = _oracle(g, tr, engine.default_options(1), np.zeros(1, np.uint32))
    edge_off, rec, shape_off, shape, merged = me.matched_edges(g, tr, ref, R=R)
    u = 110.0 + 20.0 * (float(c1) / float(c1 + m))
    want = np.array([(er, R.e_way[er], L1 - c3, L1, 100.0, u, 0, 1, 0, 3, me.NONE, 0, me.CHAIN_FIRST, L1),
                     (e2, R.e_way[e2], 0, m, u, 130.0, 1, 2, 3, 4, me.NONE, 0, 0, R.len[r2])], me.REC)
    assert edge_off.tolist() == [0, 2] and shape_off.tolist() == [0, 5] and merged == [(0, 1), (2, 2)]
    assert rec.tobytes() == want.tobytes(), (rec, want)
    one = F(1.0)
    want_shape = np.array([(R.vlon[a + 2] + one * (R.vlon[a + 3] - R.vlon[a + 2]), R.vlat[a + 2] + one * (R.vlat[a + 3] - R.vlat[a + 2])),
                           (R.vlon[a + 2], R.vlat[a + 2]), (R.vlon[a + 1], R.vlat[a + 1]), (R.vlon[a], R.vlat[a]),
                           (R.vlon[b] + one * (R.vlon[b + 1] - R.vlon[b]), R.vlat[b] + one * (R.vlat[b + 1] - R.vlat[b]))], np.float32)
    assert shape.tobytes() == want_shape.tobytes(), (shape, want_shape)


def test_abi_additions(built_lib):
    """The 64-byte record and the new calls exist in the built library and its binding; the ABI
    version and the kernel-name list are what they were."""
    import valhalla
    from reporter_amd import _lib
    assert ctypes.sizeof(_lib.RmMatchedEdge) == 64 == engine.MATCHED_EDGE_DTYPE.itemsize == me.REC.itemsize
    assert [n for n, _ in _lib.RmMatchedEdge._fields_] == list(engine.MATCHED_EDGE_DTYPE.names) == list(me.REC.names)
    assert [engine.MATCHED_EDGE_DTYPE.fields[n][1] for n in me.REC.names] == [me.REC.fields[n][1] for n in me.REC.names]
    h = ctypes.CDLL(built_lib)
    for name in ("rm_runner_matched_edges", "rm_runner_get_matched_edges", "rm_runner_matched_edges_time",
                 "rm_match_edges", "rm_match_edges_batch"):
        assert hasattr(h, name), name
    assert hasattr(engine.BatchMatcher, "matched_edges") and hasattr(engine.BatchMatcher, "matched_edges_ms")
    assert hasattr(valhalla.SegmentMatcher, "MatchEdges") and hasattr(valhalla.SegmentMatcher, "MatchEdgesMany")
    assert _lib.lib().rm_abi_version() == 1
    names = [_lib.lib().rm_kernel_name(i).decode() for i in range(_lib.lib().rm_num_kernels())]
    assert names == ["states", "candidates", "scan", "routes", "viterbi", "paths", "segments", "report", "locality", "points"]
