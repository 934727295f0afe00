"""The oracle away from 47N 8E, checked by references that share nothing with it.

At every place of tests/geo_places.py: the oracle's states, gc and candidates against the
long-double haversine and the float64 brute force of tests/geo_ref.py (the same check_* functions
run on the GPU's outputs in tests/test_gpu_geography.py), box probes at radius 5 m, the road
headings against libm's atan2, the host text readers bit for bit, and the tiles of the segment
ids.  The shares the candidate checks rest on (undecidable pairs < 1 %, qualifying probes >= 90 %)
are asserted here, on the references alone.  No GPU."""
import numpy as np
import pytest

import geo_places
import geo_ref
import lines_ref
import meili_oracle as mo
import messages_ref
import msg_text
import stream_ref as sr
from reporter_amd import engine, graphfile, world
from test_turn_penalty import _road_heads


@pytest.fixture(scope="module", params=geo_places.NAMES)
def place(request, built_lib, tmp_path_factory):
    name = request.param
    path = geo_places.build_place_world(name, str(tmp_path_factory.mktemp("geo_" + name)))
    return dict(name=name, path=path, g=graphfile.load(path), tr=geo_places.place_traces(path))


def oracle(place, tr=None, **over):
    tr = place["tr"] if tr is None else tr
    opts = engine.default_options(1, **over)
    T = len(tr["trace_off"]) - 1
    return opts, mo.match(place["g"], mo.Batch(tr["trace_off"], tr["lon"], tr["lat"], tr["time"], tr["accuracy"], opts,
                                               np.zeros(T, np.uint32)))


def candidates_of(g, tr, opts, out, every=1):
    """check_candidates on every `every`-th state of a one-option run."""
    slot, point, _ = geo_ref.state_layout(tr["trace_off"], out["n_states"], out["state_orig"])
    slot, point = slot[::every], point[::every]
    radius = geo_ref.point_radius(float(opts[0]["search_radius"]), tr["accuracy"][point])
    c = geo_ref.check_candidates(g, tr["lon"][point], tr["lat"][point], radius, geo_ref.mode_access(opts[0]["mode"]),
                                 out["cand_n"][slot], out["cand_road"][slot], out["cand_s"][slot], out["cand_sq"][slot])
    assert c["skipped"] < 0.01 * c["pairs"], c
    return c


def test_states_gc_candidates_at_radius_50(place):
    tr = place["tr"]
    opts, ref = oracle(place)
    st = geo_ref.check_states(tr["lon"], tr["lat"], tr["trace_off"], ref["n_states"], ref["state_orig"],
                              float(opts[0]["interpolation_distance"]))
    gc = geo_ref.check_gc(tr["lon"], tr["lat"], tr["trace_off"], ref["n_states"], ref["state_orig"], ref["gc"])
    c = candidates_of(place["g"], tr, opts, ref)
    print("geo", place["name"], st, gc, c)
    assert st["states"] > 600 and st["skipped"] > 100 and gc["transitions"] > 600 and gc["min_m"] < 20.0
    assert c["candidates"] > 3 * c["states"]


@pytest.mark.parametrize("case", ["r3", "r5", "r100", "acc200"])
def test_candidates_at_other_radii(place, case):
    """Radii 3, 5 and 100 m and an accuracy of 200 m (the cap), every 4th state."""
    tr = place["tr"]
    if case == "acc200":
        tr = dict(tr, accuracy=np.full(len(tr["accuracy"]), 200.0, np.float32))
        opts, ref = oracle(place, tr)
    else:
        if case in ("r3", "r5"):                        # the generator's 5 m accuracy would set the radius
            tr = dict(tr, accuracy=np.full(len(tr["accuracy"]), -1.0, np.float32))
        opts, ref = oracle(place, tr, search_radius=float(case[1:]))
    c = candidates_of(place["g"], tr, opts, ref, every=4)
    print("geo", place["name"], case, c)
    assert c["states"] > 150
    if case == "acc200":
        assert c["full_states"] > 100                   # the full-list rule is exercised
    if case in ("r3", "r5"):
        assert 0 < c["candidates"] < 2 * c["states"]    # many states with one road or none


def test_box_probes(place):
    g = place["g"]
    tr, road = geo_ref.box_probes(g)
    opts, ref = oracle(place, tr, search_radius=geo_ref.PROBE_RADIUS)
    assert (ref["n_states"] == 1).all()
    p = geo_ref.check_box_probes(g, tr, road, ref["cand_n"], ref["cand_road"])
    print("geo", place["name"], "probes", p)
    assert p["qualify"] >= 0.9, p


def test_road_headings_match_atan2(place):
    g = place["g"]
    h0, h1 = mo.road_heads(g)
    p0, p1 = _road_heads(g)
    for a, b in ((h0, p0), (h1, p1)):
        d = np.abs(a.astype(np.int64) - b)
        d = np.minimum(d, 360 - d)
        assert int(d.max()) <= 2, int(d.max())
        assert (d == 0).mean() > 0.999
    q = np.concatenate([h0, h1]).astype(np.int64)
    assert all(((q >= lo) & (q < lo + 90)).sum() > 100 for lo in (0, 90, 180, 270))   # every quadrant


def test_text_readers_read_back_bit_for_bit(place):
    """Both message kinds and the trace-file lines: the host readers and the plain-Python models
    give the arrays the text was written from."""
    arr = sr.interleave(geo_places.place_traces(place["path"], n_traces=8, n_points=100, seed=11))
    want = msg_text.expected(arr)
    fmt = msg_text.formats(engine)
    for kind in (0, 1):
        text = msg_text.text(arr, kind)
        host = engine.parse_messages_host([text], fmt[kind], strict=True)
        model = messages_ref.parse([text], fmt[kind])
        assert host["info"]["dropped"] == 0 and host["uuid"].tolist() == want["vehicle"].tolist()
        for k in ("time", "lon", "lat", "accuracy"):
            assert host[k].tobytes() == want[k].tobytes(), (kind, k)
            assert np.asarray(model[k]).astype(host[k].dtype).tobytes() == want[k].tobytes(), (kind, k)
    lines = "".join("%s,%d,%s,%s,%s\n" % (msg_text.name(int(v)), int(t), np.float32(la), np.float32(lo), np.float32(a))
                    for v, t, la, lo, a in zip(arr["vehicle"], arr["time"], arr["lat"], arr["lon"], arr["accuracy"])).encode()
    host, model = engine.parse_lines_host([lines]), lines_ref.parse([lines], engine.LineFormat())
    for k in ("time", "lon", "lat", "accuracy"):
        assert host[k].tobytes() == model[k].tobytes(), k
    assert host["lon"].tobytes() == f32bytes(arr["lon"]) and host["lat"].tobytes() == f32bytes(arr["lat"])
    lat0, lon0 = geo_places.PLACES[place["name"]]
    text = msg_text.text(arr, 0)
    if place["name"] == "null_island":
        assert (arr["lon"] < 0).any() and (arr["lat"] < 0).any() and (arr["lon"] > 0).any()
        assert sum(b"e-0" in ln for ln in text.split(b"\n")) >= 5        # exponent spellings occur
        assert sum(b",-" in ln for ln in text.split(b"\n")) > 100        # and negative values
    if lat0 < 0:
        assert (np.asarray(host["lat"]) < 0).all()
    if lon0 < 0:
        assert (np.asarray(host["lon"]) < 0).all()


def f32bytes(a):
    return np.asarray(a, np.float64).astype(np.float32).tobytes()


def _old_odd_message(arr, j, kind):
    """msg_text's odd form as it was before it learnt to leave an exponent alone."""
    v, t = int(arr["vehicle"][j]), arr["time"][j]
    lon, lat, acc = (str(np.float32(arr[k][j])) for k in ("lon", "lat", "accuracy"))
    if kind == 0:
        return " %s , %d,%se0,\t%s,%s \r" % (msg_text.name(v), int(t), lat, lon, acc)
    return ' {"nest":{"uuid":["x",{"la":"}"}]}, "lo" : %se0 , "acc":"%s","when":"%s", "uuid":"%s","la":%s}\t' % (
        lon, acc, msg_text._civil(t), msg_text.name(v), lat)


def test_msg_text_is_unchanged_at_home(built_lib, small_world):
    """At 47N 8E no coordinate is spelled with an exponent, so the odd form is byte for byte what
    it was; a spelling that has an exponent is left alone."""
    arr = sr.interleave(world.generate_traces(small_world, n_traces=8, n_points=100, rate_s=1.0, noise_m=5.0, seed=11))
    assert not any("e" in str(np.float32(x)) for k in ("lon", "lat") for x in arr[k])
    for kind in (0, 1):
        for j in range(len(arr["vehicle"])):
            assert msg_text.message(arr, j, kind, True) == _old_odd_message(arr, j, kind)
    near = {"vehicle": np.array([1]), "time": np.array([101.0]), "lon": np.array([4.2e-05]), "lat": np.array([-1.5e-05]),
            "accuracy": np.array([5.0], np.float32)}
    assert msg_text.message(near, 0, 0, True) == " veh/001-bus , 101,-1.5e-05,\t4.2e-05,5.0 \r"
    assert '"lo" : 4.2e-05 ,' in msg_text.message(near, 0, 1, True)


def test_segment_ids_name_the_tile_of_the_first_node(place):
    g = place["g"]
    size = {0: 4.0, 1: 1.0, 2: 0.25}
    ids = g["seg_id"].astype(np.uint64)
    assert len(ids) > 50
    first = np.nonzero((g["edge_seg"] != geo_ref.NONE) & (g["edge_seg_off"] == 0))[0]
    seg = g["edge_seg"][first]
    assert sorted(seg.tolist()) == list(range(len(ids)))              # one first edge per segment
    node = np.searchsorted(g["node_off"], first, side="right") - 1
    files = set()
    for s, n in zip(seg.tolist(), node.tolist()):
        level, tile = int(ids[s]) & 7, (int(ids[s]) >> 3) & 0x3FFFFF
        lat, lon = float(g["node_lat"][n]), float(g["node_lon"][n])
        ncols = int(round(360.0 / size[level]))
        row, col = int(np.floor((lat + 90.0) / size[level])), int(np.floor((lon + 180.0) / size[level]))
        assert tile == row * ncols + col, (s, level, tile, lat, lon)
        assert 0 <= col < ncols and 0 <= row < int(round(180.0 / size[level]))
        files.add(world.valhalla_tile_file(level, tile))
    assert files == set(world.valhalla_tiles(place["path"]).values())
    for f in files:
        parts = f[:-4].split("/")
        assert f.endswith(".gph") and parts[0] in "012" and all(len(p) == 3 and p.isdigit() for p in parts[1:]), f
