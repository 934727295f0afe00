"""Which walker wrote a long path and which summed a tie's turn weight, at a small shape (GPU).

A route's canonical path is walked by the path stage (its edges) and by the routes stage (its turn
weights, DESIGN.md §3 rule 3b), through the route tables or through a search tier's labels.  The
parity suites compare every path edge and every distance term with the oracle; these runs pin, on
two hand-written graphs, that a path longer than the eight inline edges came from the walker named,
and that the tables' turn walk (k_turn_walks) is certain to run.

Both graphs are a zigzag chain of 34 two-node residential ways: node i at lon i * 0.000539,
lat 0.0003 * (i & 1), so every road is 6,856 cm long and every joint a graph node with a bend.

One-way chain: traces of four points, 150 s apart, on roads r, r + 10, r + 20, r + 30.  Every
transition's path has 11 edges (the pool, not the inline slots) and every route a turn weight.
Only r = 1, 2, 3 keep such a trace inside the chain, so the batch repeats them at twelve offsets
along the road (36 traces, 144 points).  With 1,000 m tables the table walker writes the pool
paths; without tables a path needs at least eight labels, which overflows the 7-label lane tier,
and on a one-way chain the search labels only the nodes between source and target, which fit the
12-label second tier.

Two-way chain: traces of eleven points, 40 s apart, exactly on nodes n, n + 3, ... (n = 1, 2, 3).
Every candidate sits at an end of its road (s = 0 or s = 6856).  Such a source ties its two exits at
the target's entry node (the route from the far exit runs back along the source road), a tie has no
turn row to read (k2_turn_key: need 2), so with 500 m tables K2 lists these routes for k_turn_walks, which
walks them through the tables.  No counter shows that walk; the listing follows from the tie.

Dense two-way chain: the same chain at half the spacing (node i at lon i * 0.00027, lat 0.00015 *
(i & 1), roads of 3,433 cm) under a 200 m search radius, six traces of ten points on nodes n, n + 3,
...  Up to 14 candidates a point, all at road ends, give so many tied routes that some K2 block lists
more than kWalkPerBlock = 512 of them whatever the item order: the rest are marked in place and
walked by k_turn_walks_marked.
"""
import numpy as np
import pytest

import meili_oracle as mo
from parity_util import compare_all
from reporter_amd import engine, graphfile, world

pytestmark = pytest.mark.gpu

N_WAYS = 34
DLON, DLAT = 0.000539, 0.0003
ROAD_CM = 6856

_cache = {}


DENSE = (0.00027, 0.00015)   # the dense chain's node spacing
DENSE_ROAD_CM = 3433
WALK_PER_BLOCK, K2_ITEMS = 512, 256   # engine.hip kWalkPerBlock, kK2Items


def _node(i, d=(DLON, DLAT)):
    return i * d[0], d[1] * (i & 1)


def _chain_osm(oneway, d=(DLON, DLAT)):
    rows = ["<?xml version='1.0' encoding='UTF-8'?>", '<osm version="0.6" generator="hand">']
    for i in range(N_WAYS + 1):
        lon, lat = _node(i, d)
        rows.append(' <node id="%d" lat="%.7f" lon="%.7f"/>' % (i + 1, lat, lon))
    for k in range(N_WAYS):
        rows.append(' <way id="%d">' % (100 + k))
        rows.append('  <nd ref="%d"/><nd ref="%d"/>' % (k + 1, k + 2))
        rows.append('  <tag k="highway" v="residential"/>')
        if oneway:
            rows.append('  <tag k="oneway" v="yes"/>')
        rows.append(' </way>')
    rows.append("</osm>")
    return "\n".join(rows) + "\n"


def _traces(points, dt):
    """A batch from per-trace lists of (lon, lat), `dt` seconds between a trace's points."""
    lens = [len(p) for p in points]
    flat = np.array([q for p in points for q in p], np.float64)
    return dict(trace_off=np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32),
                lon=flat[:, 0].astype(np.float32), lat=flat[:, 1].astype(np.float32),
                time=np.concatenate([1_500_000_000.0 + dt * np.arange(n) for n in lens]),
                accuracy=np.full(len(flat), 5.0, np.float32))


def _on_road(k, f):
    (x0, y0), (x1, y1) = _node(k), _node(k + 1)
    return x0 + f * (x1 - x0), y0 + f * (y1 - y0)


def _oneway_traces():
    fracs = (0.5, 0.3, 0.34, 0.38, 0.42, 0.46, 0.54, 0.58, 0.62, 0.66, 0.7, 0.74)   # the mid-point first
    return _traces([[_on_road(r + 10 * q, f) for q in range(4)] for f in fracs for r in (1, 2, 3)], 150.0)


def _twoway_traces():
    return _traces([[_node(n + 3 * q) for q in range(11)] for n in (2, 1, 3)], 40.0)


def _case(built_lib, tmpdir_session, oneway):
    """Graph, batch and the oracle's answer: computed once, shared by the tests, left unchanged."""
    if oneway not in _cache:
        name = "walk_oneway" if oneway else "walk_twoway"
        osm = tmpdir_session / (name + ".osm")
        osm.write_text(_chain_osm(oneway))
        path = world.import_osm(str(osm), str(tmpdir_session / (name + ".rmg")), cell_m=50.0)
        g = graphfile.load(path)
        assert len(g["road_len_cm"]) == N_WAYS and (np.asarray(g["road_len_cm"]) == ROAD_CM).all()
        tr = _oneway_traces() if oneway else _twoway_traces()
        assert int(tr["trace_off"][-1]) < 1000
        opts = engine.default_options(1, turn_penalty_factor=200.0)
        T = len(tr["trace_off"]) - 1
        ref = mo.match(g, mo.Batch(tr["trace_off"], tr["lon"], tr["lat"], tr["time"], tr["accuracy"], opts,
                                   np.zeros(T, np.uint32)))
        _cache[oneway] = (path, tr, opts, ref)
    return _cache[oneway]


def _run(path, tr, opts, radius):
    eng = engine.Engine(path, 0)
    eng.set_ball_radius(radius)
    bm = engine.BatchMatcher(eng)
    T = len(tr["trace_off"]) - 1
    bm.run(tr["trace_off"], tr["lon"], tr["lat"], tr["time"], tr["accuracy"], opts, np.zeros(T, np.uint32))
    return eng, bm


def _turned(ref):
    valid = ref["route"] != 0xffffffff
    return int((ref["route_turn"][valid] > 0).sum())


def test_oneway_long_paths_from_the_tables(built_lib, tmpdir_session):
    """1,000 m tables answer every transition, so the table walker filled the pool paths."""
    path, tr, opts, ref = _case(built_lib, tmpdir_session, True)
    eng, bm = _run(path, tr, opts, 1000.0)
    tiers = bm.route_tiers()
    print("one-way, 1000 m tables", tiers, "path_cnt max", int(ref["path_cnt"].max()), "turned", _turned(ref))
    c = compare_all(bm, ref, tr["trace_off"])
    assert tiers["paths_ball_to_search"] == 0, tiers
    assert (ref["path_cnt"] > 8).any()
    assert c["chained"] >= 3 and _turned(ref) > 0, c
    bm.close()
    eng.close()


@pytest.mark.parametrize("small", [False, True], ids=["ordinary", "small"])
def test_oneway_long_paths_from_the_second_tier(built_lib, tmpdir_session, monkeypatch, small):
    """No tables: the paths overflow the lane tier and the second register tier writes them (none
    reaches the group tier); the routes' turn weights come from the search tiers' walk.  Once on the
    ordinary run path and once on the small one."""
    if small:
        monkeypatch.delenv("RM_SMALL_BATCH_POINTS", raising=False)
    else:
        monkeypatch.setenv("RM_SMALL_BATCH_POINTS", "0")
    path, tr, opts, ref = _case(built_lib, tmpdir_session, True)
    eng, bm = _run(path, tr, opts, 0.0)
    tiers, sizes = bm.route_tiers(), bm.sizes()
    print("one-way, no tables, small %s" % small, tiers, "paths_tier2", sizes["paths_tier2"])
    compare_all(bm, ref, tr["trace_off"])
    assert sizes["paths_tier2"] > 0, sizes
    assert tiers["paths_group_to_wave512"] == 0, tiers
    assert (ref["path_cnt"] > 8).any() and _turned(ref) > 0
    bm.close()
    eng.close()


@pytest.mark.parametrize("radius", [500.0, 0.0], ids=["balls500", "radius0"])
def test_twoway_tied_exits_walk_the_tables(built_lib, tmpdir_session, radius):
    """Sources at road ends tie their exits: with 500 m tables every route is the tables' and its
    turn weight the table walk's; without tables the search tiers' walk gives the same."""
    path, tr, opts, ref = _case(built_lib, tmpdir_session, False)
    sm = np.zeros(len(ref["cand_n"]), bool)
    for k in range(len(tr["trace_off"]) - 1):
        o = int(tr["trace_off"][k])
        sm[o:o + int(ref["n_states"][k])] = True
    live = (np.arange(16)[None, :] < ref["cand_n"][:, None]) & sm[:, None]
    assert live.any() and np.isin(ref["cand_s"][live], (0, ROAD_CM)).all()   # every source ties its exits
    eng, bm = _run(path, tr, opts, radius)
    tiers = bm.route_tiers()
    print("two-way, radius %g" % radius, tiers, "turned", _turned(ref))
    c = compare_all(bm, ref, tr["trace_off"])
    if radius:
        assert tiers["ball_to_search"] == 0, tiers
    assert c["chained"] >= 10 and _turned(ref) > 0, c
    bm.close()
    eng.close()


def _dense_case(built_lib, tmpdir_session):
    if "dense" not in _cache:
        osm = tmpdir_session / "walk_dense.osm"
        osm.write_text(_chain_osm(False, DENSE))
        path = world.import_osm(str(osm), str(tmpdir_session / "walk_dense.rmg"), cell_m=50.0)
        g = graphfile.load(path)
        assert len(g["road_len_cm"]) == N_WAYS and (np.asarray(g["road_len_cm"]) == DENSE_ROAD_CM).all()
        # road ids ascend along the chain (what "further along" below means)
        west = np.minimum(g["node_lon"][g["road_node0"]], g["node_lon"][g["road_node1"]])
        assert (np.diff(west) > 0).all()
        tr = _traces([[_node(n + 3 * q, DENSE) for q in range(10)] for n in (2, 1, 3, 2, 1, 3)], 40.0)
        opts = engine.default_options(1, turn_penalty_factor=200.0, search_radius=200.0)
        T = len(tr["trace_off"]) - 1
        ref = mo.match(g, mo.Batch(tr["trace_off"], tr["lon"], tr["lat"], tr["time"], tr["accuracy"], opts,
                                   np.zeros(T, np.uint32)))
        _cache["dense"] = (path, tr, opts, ref)
    return _cache["dense"]


def _tied_routes(tr, ref):
    """(items, tied) from the reference alone: the (pair, source) items K2 takes, and the valid routes
    from a source at s == 0 to a road further along the chain or from one at s == length to a road
    further back -- the far exit's route runs back along the source road, so both exits give the
    entry node the same label."""
    items = tied = 0
    for k in range(len(tr["trace_off"]) - 1):
        o = int(tr["trace_off"][k])
        for p in range(o + 1, o + int(ref["n_states"][k])):
            ka, kb = int(ref["cand_n"][p - 1]), int(ref["cand_n"][p])
            items += ka
            route = ref["route"][int(ref["trans_off"][p]):][:ka * kb].reshape(ka, kb)
            src_road, src_s = ref["cand_road"][p - 1, :ka, None], ref["cand_s"][p - 1, :ka, None]
            dst_road = ref["cand_road"][p, None, :kb]
            tie = ((src_s == 0) & (dst_road > src_road)) | ((src_s == DENSE_ROAD_CM) & (dst_road < src_road))
            tied += int((tie & (route != 0xffffffff)).sum())
    return items, tied


@pytest.mark.parametrize("small", [False, True], ids=["ordinary", "small"])
def test_dense_twoway_overflows_a_block_walk_list(built_lib, tmpdir_session, monkeypatch, small):
    """More tied routes than all K2 blocks can list (512 each): some block's list overflows, its
    further walks are marked in place and k_turn_walks_marked walks them.  Every route is the
    tables' and every distance term the oracle's, on the ordinary run path and on the small one."""
    if small:
        monkeypatch.delenv("RM_SMALL_BATCH_POINTS", raising=False)
    else:
        monkeypatch.setenv("RM_SMALL_BATCH_POINTS", "0")
    path, tr, opts, ref = _dense_case(built_lib, tmpdir_session)
    items, tied = _tied_routes(tr, ref)
    blocks = -(-items // K2_ITEMS)
    print("dense two-way, small %s: points %d items %d blocks %d tied %d cand_n max %d" %
          (small, int(tr["trace_off"][-1]), items, blocks, tied, int(ref["cand_n"].max())))
    assert tied > WALK_PER_BLOCK * blocks, (items, tied)
    eng, bm = _run(path, tr, opts, 1000.0)
    tiers = bm.route_tiers()
    print(tiers)
    c = compare_all(bm, ref, tr["trace_off"])
    assert tiers["ball_to_search"] == 0, tiers
    assert c["chained"] == int(tr["trace_off"][-1]) - (len(tr["trace_off"]) - 1), c   # every transition chained
    bm.close()
    eng.close()
