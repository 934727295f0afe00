"""The GPU stages away from 47N 8E: negative and near-zero coordinates, longitudes
at both ends of the range, the equator and 78N (tests/geo_places.py).

At every place the engine is compared with the oracle stage by stage (plain, with turn costs, and a
set that mixes modes and search radii), and its own states, gc and candidates are checked by the
references of tests/geo_ref.py, which share no code and no float32 frame with either; the truth
recovery must not fall below home's.  At the places with negative or near-zero coordinates the
matched points and edges (records and JSON replies), the stream from raw messages to tile files and
the batch lines path run the checks of their own test modules.

K1 has two kernels.  A batch of at most 4096 points takes the small run with one wave per state
(k_candidates_wave alone); any other run takes the lane kernel (k_candidates_lane / k1_gather, the
production K1 with its own padded box, cell arithmetic and row windows) and hands states with more
than 16 roads to the wave kernel.  The sets here are small, so the parity and reference tests run
twice (fixture `k1`): as they come ("wave") and on the ordinary run path, RM_SMALL_BATCH_POINTS=0
("lane").  The reference test asserts which kernel ran by the lane kernel's hand-over count; the
parity tests go through match_and_compare, which keeps its runner, so there the kernel follows from
the batch size (asserted) and the environment rule.  The 32 x 300 recovery set (9600 points) takes the small run with the lane kernel and is
checked by the references too."""
import json
import re

import numpy as np
import pytest

import geo_places
import geo_ref
from parity_util import match_and_compare, truth_recovery
from reporter_amd import engine, graphfile, world

pytestmark = pytest.mark.gpu

MODES = ("auto", "bicycle", "pedestrian")
RADII = (5.0, 50.0, 100.0)
NEGATIVE_OR_ZERO = ("san_francisco", "ushuaia", "null_island", "fiji")


@pytest.fixture(scope="module")
def worlds(built_lib, tmp_path_factory):
    """name -> path of the place's 24 x 24 world, built once."""
    d, made = str(tmp_path_factory.mktemp("geo")), {}

    def get(name):
        if name not in made:
            made[name] = geo_places.build_place_world(name, d)
        return made[name]
    return get


@pytest.fixture(scope="module", params=geo_places.NAMES)
def site(request, worlds):
    """One engine per place."""
    path = worlds(request.param)
    eng = engine.Engine(path, 0)
    yield dict(name=request.param, path=path, g=graphfile.load(path), tr=geo_places.place_traces(path), eng=eng)
    eng.close()


WAVE_K1_POINTS = 4096      # engine.hip kSmallWaveK1: the small run gives K1 a wave per state up to here


@pytest.fixture(params=["wave", "lane"])
def k1(request, monkeypatch):
    """Which K1 kernel the test's runs take: "wave" as small batches come, "lane" on the ordinary
    run path (the suite's idiom: test_gpu_small.py, test_gpu_k1_epilogue.py)."""
    if request.param == "lane":
        monkeypatch.setenv("RM_SMALL_BATCH_POINTS", "0")
    else:
        monkeypatch.delenv("RM_SMALL_BATCH_POINTS", raising=False)
    return request.param


def mixed_set(path):
    """12 traces: auto, bicycle and pedestrian, each with search radii 5, 50 and 100 m.  240 points
    each: at 120 the 5 m rows leave one complete segment traversal per place or none (Sydney), and
    match_and_compare wants a speed histogram that is not empty; 240 leave six everywhere."""
    opts = engine.default_options(9)
    for m, mode in enumerate(MODES):
        for k, r in enumerate(RADII):
            opts[3 * m + k]["mode"] = world.MODES[mode]
            opts[3 * m + k]["search_radius"] = r
    tr = world.concat_traces(*[geo_places.place_traces(path, 4, 240, seed=21 + m, mode=mode) for m, mode in enumerate(MODES)])
    topt = np.array([3 * (k // 4) + k % 3 for k in range(12)], np.uint32)
    return tr, opts, topt


@pytest.mark.parametrize("turns", [0.0, 200.0])
def test_matcher_equals_oracle(site, turns, k1):
    assert len(site["tr"]["lon"]) <= WAVE_K1_POINTS
    c = match_and_compare(site["path"], site["tr"], engine.default_options(1, turn_penalty_factor=turns), None, hist=True)
    assert c["traces"] == 12 and c["segments"] > 50 and c["valid_reports"] > 0, c
    print("geo parity", site["name"], k1, turns, c)


def test_mixed_modes_and_radii_equal_oracle(site, k1):
    """The batch radius is 100 m: every row goes through the second K1 grid where there is one."""
    tr, opts, topt = mixed_set(site["path"])
    assert len(tr["lon"]) <= WAVE_K1_POINTS
    c = match_and_compare(site["path"], tr, opts, topt, hist=True)
    assert c["traces"] == 12 and c["segments"] > 30, c
    print("geo mixed parity", site["name"], k1, "grid", site["eng"].grid_split(), site["eng"].grid_alt(), c)


def test_some_place_uses_a_second_k1_grid(worlds):
    alt = {}
    for name in geo_places.NAMES:
        eng = engine.Engine(worlds(name), 0)
        alt[name] = (eng.grid_split(),) + eng.grid_alt()
        eng.close()
    print("geo grids (split, second split, from radius)", alt)
    assert any(f not in (0, s) and r <= 100.0 for s, f, r in alt.values()), alt


def _run(site, tr, opts, topt=None):
    bm = engine.BatchMatcher(site["eng"])
    bm.run(tr["trace_off"], tr["lon"], tr["lat"], tr["time"], tr["accuracy"], opts, topt)
    n_states, orig = bm.states()
    out = dict(n_states=n_states, state_orig=orig, gc=bm.routes()[1])
    out["cand_n"], out["cand_road"], out["cand_s"], out["cand_sq"] = bm.candidates()
    out["choice"] = bm.viterbi()[0]
    out["points"] = len(tr["lon"])
    out["lane_to_wave"] = bm.sizes()["cand_tier2"]   # states the lane kernel handed to the wave kernel
    bm.close()
    return out


def _assert_k1_tier(k1, outs):
    """The runs took the K1 kernel the test is named for.  A wave-per-state run never counts a
    hand-over; of the lane runs, the 200 m one (more than 16 roads around most states) must."""
    if k1 == "wave":
        assert all(o["points"] <= WAVE_K1_POINTS and o["lane_to_wave"] == 0 for o in outs.values()), \
            {k: (o["points"], o["lane_to_wave"]) for k, o in outs.items()}
    else:
        assert outs["acc200"]["lane_to_wave"] > 100 and outs["r3"]["lane_to_wave"] == 0, \
            {k: o["lane_to_wave"] for k, o in outs.items()}


def _check_candidates(g, tr, opts, topt, out, every=1):
    slot, point, trace = geo_ref.state_layout(tr["trace_off"], out["n_states"], out["state_orig"])
    slot, point, trace = slot[::every], point[::every], trace[::every]
    o = opts[np.zeros(len(tr["trace_off"]) - 1, np.int64) if topt is None else topt.astype(np.int64)][trace]
    radius = geo_ref.point_radius(o["search_radius"], tr["accuracy"][point])
    access = np.array([geo_ref.mode_access(m) for m in o["mode"]])
    c = geo_ref.check_candidates(g, tr["lon"][point], tr["lat"][point], radius, access, out["cand_n"][slot],
                                 out["cand_road"][slot], out["cand_s"][slot], out["cand_sq"][slot])
    assert c["skipped"] < 0.01 * c["pairs"], c
    return c


def test_references_on_the_gpus_own_outputs(site, k1):
    """check_states, check_gc and check_candidates (radius 50 m: every state; radii 3, 5, 100 m, an
    accuracy of 200 m and the mixed set: every 4th) and the box probes on BatchMatcher's outputs,
    once per K1 kernel."""
    g, tr = site["g"], site["tr"]
    opts = engine.default_options(1)
    outs = {}
    out = outs["r50"] = _run(site, tr, opts)
    st = geo_ref.check_states(tr["lon"], tr["lat"], tr["trace_off"], out["n_states"], out["state_orig"],
                              float(opts[0]["interpolation_distance"]))
    gc = geo_ref.check_gc(tr["lon"], tr["lat"], tr["trace_off"], out["n_states"], out["state_orig"], out["gc"])
    c = _check_candidates(g, tr, opts, None, out)
    print("geo gpu", site["name"], k1, st, gc, c)
    assert st["states"] > 600 and st["skipped"] > 100 and gc["transitions"] > 600 and c["candidates"] > 3 * c["states"]
    no_acc = dict(tr, accuracy=np.full(len(tr["accuracy"]), -1.0, np.float32))
    wide = dict(tr, accuracy=np.full(len(tr["accuracy"]), 200.0, np.float32))
    for case, t, o in (("r3", no_acc, engine.default_options(1, search_radius=3.0)),
                       ("r5", no_acc, engine.default_options(1, search_radius=5.0)),
                       ("r100", tr, engine.default_options(1, search_radius=100.0)), ("acc200", wide, opts)):
        outs[case] = _run(site, t, o)
        c = _check_candidates(g, t, o, None, outs[case], every=4)
        print("geo gpu", site["name"], k1, case, c)
        assert c["states"] > 150 and (case != "acc200" or c["full_states"] > 100)
    mtr, mopts, mtopt = mixed_set(site["path"])
    mout = outs["mixed"] = _run(site, mtr, mopts, mtopt)
    geo_ref.check_gc(mtr["lon"], mtr["lat"], mtr["trace_off"], mout["n_states"], mout["state_orig"], mout["gc"])
    c = _check_candidates(g, mtr, mopts, mtopt, mout, every=4)
    print("geo gpu", site["name"], k1, "mixed", c)
    ptr, road = geo_ref.box_probes(g)
    pout = outs["probes"] = _run(site, ptr, engine.default_options(1, search_radius=geo_ref.PROBE_RADIUS))
    assert (pout["n_states"] == 1).all()
    p = geo_ref.check_box_probes(g, ptr, road, pout["cand_n"], pout["cand_road"])
    print("geo gpu", site["name"], k1, "probes", p)
    assert p["qualify"] >= 0.9, p
    _assert_k1_tier(k1, outs)


def _recovery(path, eng):
    """Truth recovery of the GPU's own choices on 32 x 300 points: (rate, matched states).  9600
    points: the small run with the lane kernel, so its gc and (every 4th state) candidates go
    through the references as well."""
    tr = geo_places.place_traces(path, 32, 300, seed=31)
    opts = engine.default_options(1)
    out = _run(dict(eng=eng), tr, opts)
    assert out["points"] > WAVE_K1_POINTS
    g = graphfile.load(path)
    gc = geo_ref.check_gc(tr["lon"], tr["lat"], tr["trace_off"], out["n_states"], out["state_orig"], out["gc"])
    c = _check_candidates(g, tr, opts, None, out, every=4)
    print("geo gpu recovery set", path.rsplit("/", 1)[-1], gc, c)
    assert c["states"] > 1500 and c["candidates"] > 3 * c["states"]
    rate, matched, states = truth_recovery(tr["trace_off"], out["n_states"], out["state_orig"], out["cand_road"],
                                           out["choice"], tr["truth_edge"], g["edges"])
    assert matched > 0.9 * states > 5000
    return rate, matched


@pytest.fixture(scope="module")
def home_recovery(worlds):
    eng = engine.Engine(worlds(geo_places.HOME), 0)
    r = _recovery(worlds(geo_places.HOME), eng)
    eng.close()
    return r


def test_truth_recovery_is_homes(site, home_recovery):
    """The share of matched states on the road the generator drove is no lower than at 47N 8E on
    the same seeds, less 4 sigma of home's binomial (4: ten places are compared)."""
    p, n = home_recovery
    margin = 4.0 * np.sqrt(p * (1.0 - p) / n)
    rate, matched = _recovery(site["path"], site["eng"])
    print("geo truth", site["name"], "rate %.4f of %d; home %.4f of %d; margin %.4f" % (rate, matched, p, n, margin))
    assert p > 0.9
    assert rate >= p - margin, (rate, p, margin)


def _digits(text):
    """The significant digits of a decimal spelling, without sign, point, exponent and outer zeros."""
    return re.sub(r"[eE].*", "", text).replace("-", "").replace("+", "").replace(".", "").strip("0")


def check_coordinate_text(reply, rec, lon_in, lat_in):
    """The spelling of every lat / lon of a MatchPoints reply, which check_reply compares as parsed
    values only: the text reads back to the record's float32 bit for bit (sign of zero included),
    carries exactly the shortest digits that do so, and nothing but a JSON number.  The repository
    has no byte-level reference of the reply; this is the text-level part that has one.  Returns
    the tokens spelled with an exponent."""
    toks = re.findall(r'\{"lat":([^,}]+),"lon":([^,}]+),"type"', reply)
    assert len(toks) == len(rec)
    expo = []
    for (la, lo), r, x, y in zip(toks, rec, lon_in, lat_in):
        want = (r["lat"], r["lon"]) if r["type"] != 0 else (np.float32(y), np.float32(x))
        for tok, w in zip((la, lo), want):
            assert re.fullmatch(r"-?(0|[1-9][0-9]*)(\.[0-9]+)?([eE][-+]?[0-9]+)?", tok), tok
            assert np.float32(tok).tobytes() == np.float32(w).tobytes(), (tok, w)
            assert _digits(tok) == _digits(np.format_float_scientific(np.float32(w), unique=True)), (tok, w)
            if "e" in tok.lower():
                expo.append(tok)
    return expo


@pytest.mark.parametrize("name", NEGATIVE_OR_ZERO)
def test_matched_points_and_edges(worlds, name, tmp_path):
    """matched_points() / matched_edges() against their restatements, and the MatchPoints / MatchEdges
    replies against the records.  check_reply of either module compares the replies' parsed fields
    with the records (coordinates as float32 values, the precision-6 polyline as integers): the
    strongest check the repository has, there being no byte-level reference of a reply.  The
    spelling of the coordinates (exponent form near 0 degrees, signs) is checked on the text by
    check_coordinate_text, for all twelve traces."""
    import valhalla
    import test_gpu_matched_edges as te
    import test_gpu_matched_points as tp
    path = worlds(name)
    g = graphfile.load(path)
    tr = geo_places.place_traces(path, 12, 60, seed=301)
    opts = engine.default_options(1)
    rec, _ = tp.run_and_compare(path, tr, opts, what=name)
    (eo, erec, so, sh), _, _, _ = te.run_and_compare(path, tr, opts, what=name)
    assert (rec["type"] == 1).sum() > 200 and (rec["type"] == 2).sum() > 50 and len(erec) > 100
    lat0, lon0 = geo_places.PLACES[name]
    m = rec["type"] != 0
    assert lat0 >= 0 or (rec["lat"][m] < 0).all()
    assert lon0 >= 0 or (rec["lon"][m] < 0).all()
    if name == "null_island":
        assert (rec["lon"][m] < 0).any() and (rec["lon"][m] > 0).any() and (np.abs(rec["lat"][m]) < 1e-4).any()
    valhalla.Configure(valhalla.write_config(str(tmp_path / "geo.json"), path, device=0))
    sm = valhalla.SegmentMatcher()
    reqs = [json.dumps(world.trace_to_request(tr, k), separators=(",", ":")) for k in range(3)]
    pts = [sm.MatchPoints(reqs[0])] + sm.MatchPointsMany(reqs[1:])
    eds = [sm.MatchEdges(reqs[0])] + sm.MatchEdgesMany(reqs[1:])
    elen = g["edges"].reshape(-1, 4)[:, 1]
    for k in range(3):
        o = int(tr["trace_off"][k])
        plain = sm.Match(reqs[k])
        tp.check_reply(pts[k], plain, rec[o:o + 60], tr["lon"][o:o + 60], tr["lat"][o:o + 60], elen)
        rep = te.check_reply(eds[k], plain, erec[eo[k]:eo[k + 1]], sh[so[k]:so[k + 1]], g["seg_id"])
        assert len(rep["edges"]) > 3
    expo = []
    for k, reply in enumerate(sm.MatchPointsMany([json.dumps(world.trace_to_request(tr, k), separators=(",", ":"))
                                                   for k in range(12)])):
        o = int(tr["trace_off"][k])
        expo += check_coordinate_text(reply, rec[o:o + 60], tr["lon"][o:o + 60], tr["lat"][o:o + 60])
    print("geo reply text", name, "exponent spellings", expo[:6], len(expo))
    if name == "null_island":
        assert any(re.fullmatch(r"-?[0-9](\.[0-9]+)?e-0[0-9]", t) for t in expo) and any(t.startswith("-") for t in expo), expo
    else:
        assert not expo
    sm.close()


@pytest.mark.parametrize("name", ["null_island", "san_francisco", "fiji"])
def test_stream_messages_to_tiles(worlds, name):
    """test_gpu_stream's end-to-end check (windows, reports, directory indices, flushed CSV against
    the models), both message kinds, 16 vehicles x 200 points in 20 s pushes."""
    import test_gpu_stream as ts
    path = worlds(name)
    ctx = ts.make_ctx(path, geo_places.place_traces(path, 16, 200, seed=11), 16)
    try:
        # not vacuous (the oracle-driven models give 13-14 + 7-9 reports and 20-23 kept rows at these
        # places): reports from the pushes and from the final punctuate, and rows that survive the
        # privacy cull in the files, which messages_to_tiles asserts to be the GPU's byte for byte
        anon = ts.ar.Anonymiser(ts.Q, 2)
        anon.add(ctx["segs"])
        files, counts = anon.flush()
        print("geo stream", name, "pushed", ctx["n_push"], "reports", len(ctx["segs"]), counts)
        assert ctx["n_push"] >= 10 and len(ctx["segs"]) - ctx["n_push"] >= 5
        assert counts["rows_kept"] >= 15 and counts["rows_in"] > counts["rows_kept"] and len(files) >= 5
        for kind in (0, 1):
            pushed, punctuated = ts.messages_to_tiles(ctx, kind, "20s", 2)
            assert (pushed, punctuated) == (ctx["n_push"], len(ctx["segs"]) - ctx["n_push"])
    finally:
        ts.close_ctx(ctx)


@pytest.mark.parametrize("name", ["null_island", "ushuaia"])
def test_batch_lines_path(worlds, name, tmp_path):
    """test_gpu_lines' run_lines-equals-run_points check: signed and near-zero coordinates as text."""
    import test_gpu_lines as tl
    path = worlds(name)
    case = tl.make_stream_case(path, tmp_path)
    assert (case["pts"]["lon"] < 0).any() and (case["pts"]["lat"] < 0).any()
    tl.run_lines_equals_run_points(path, case)


def test_osm_city_at_sydney(built_lib, tmp_path, k1):
    """The irregular city (curved ways, one-way pairs) south of the equator, auto and pedestrian,
    once per K1 kernel."""
    city = geo_places.build_place_city("sydney", str(tmp_path))
    g = graphfile.load(city)
    assert (g["node_lat"] < 0).all() and (g["node_lon"] > 151).all()
    tr = world.concat_traces(world.generate_traces(city, 20, 60, rate_s=1.0, noise_m=5.0, seed=81, mode="auto"),
                             world.generate_traces(city, 20, 60, rate_s=1.0, noise_m=5.0, seed=82, mode="pedestrian"))
    opts = engine.default_options(2)
    opts[1]["mode"] = world.MODES["pedestrian"]
    c = match_and_compare(city, tr, opts, np.repeat(np.arange(2, dtype=np.uint32), 20), rl=(0, 1, 2), tl=(0, 1, 2), hist=True)
    assert c["traces"] == 40 and c["segments"] > 100, c
    print("geo city sydney", k1, c)
