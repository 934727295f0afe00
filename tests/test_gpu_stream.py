"""The streaming topology end to end on the GPU (DESIGN.md §3 rules 12 to 14): raw messages ->
directory -> sessions -> tile store -> CSV bytes.  push_messages must give, call by call and bit for
bit, the windows and forwarded reports of VehicleSessions.push fed the host reader's arrays and the
directory model's indices, which are the session model's (tests/stream_ref.py); the flushed files
must be the anonymiser model's (tests/anonymiser_ref.py) byte for byte; and python -m
reporter_amd.stream over the same text must write exactly those files.

Inputs (checked on the CPU with the two models alone): conftest's small_world, the traces and the
set-B thresholds of test_gpu_sessions.py (32 vehicles x 400 points at 1 Hz, seed 11; 1200 m / 20 /
150 s), the arrivals written as text by tests/msg_text.py and read back by the host reader: 80
reports forwarded by the pushes and 8 more by the final punctuate."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import anonymiser_ref as ar
import messages_ref
import msg_text
import stream_ref as sr
from reporter_amd import engine, graphfile, world

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B_PARAMS = dict(dist=1200.0, count=20, time_s=150.0)
Q = 60
SPEC = {0: "@sv@,@0@2@3@1@4", 1: "@json@uuid@la@lo@when@acc@yyyy-MM-dd HH:mm:ss"}


def make_ctx(path, tr, n_vehicles):
    """The inputs of the end-to-end run on the graph at `path`: the traces' arrivals, what their text
    reads back to per kind (host reader, directory model), the session and anonymiser models' reports,
    and an engine with a runner (close_ctx closes them)."""
    g = graphfile.load(path)
    arr = sr.interleave(tr)
    fmt = msg_text.formats(engine)
    # what the messages read back to, by the host reader and the directory model, per kind
    pts = {}
    for kind in (0, 1):
        text = msg_text.text(arr, kind)
        host = engine.parse_messages_host([text], fmt[kind], strict=True)
        ref = messages_ref.parse([text], fmt[kind])
        host["vehicle"] = messages_ref.Directory(n_vehicles).assign(ref["point_names"])
        host["stamp_ms"] = (host["time"] * 1000.0).astype(np.int64)
        pts[kind] = host
    ts = int(arr["time"].max() * 1000) + 10 ** 7
    p = pts[0]
    model = sr.Sessions(n_vehicles, sr.oracle_matcher(g, engine.default_options(1)), **B_PARAMS)
    model.push(p["vehicle"], p["time"], p["lon"], p["lat"], p["accuracy"], p["stamp_ms"])
    n_push, n_win_push = len(model.reports), len(model.windows)
    model.punctuate(ts)
    segs = [(int(r["id"]), int(r["next_id"]), float(r["t0"]), float(r["t1"]), int(r["length"]), int(r["queue_length"]))
            for r, _, _ in model.reports]
    eng = engine.Engine(path, 0)
    bm = engine.BatchMatcher(eng)
    return {"arr": arr, "fmt": fmt, "pts": pts, "ts": ts, "model": model, "n_push": n_push, "n_win_push": n_win_push,
            "segs": segs, "eng": eng, "bm": bm, "path": path, "n": n_vehicles}


def close_ctx(ctx):
    ctx["bm"].close()
    ctx["eng"].close()


@pytest.fixture(scope="module")
def ctx(built_lib, small_world):
    tr = world.generate_traces(small_world, n_traces=32, n_points=400, rate_s=1.0, noise_m=5.0, seed=11)
    c = make_ctx(small_world, tr, 32)
    yield c
    close_ctx(c)


def _session(ctx):
    return engine.VehicleSessions(ctx["bm"], ctx["n"], report_dist_m=B_PARAMS["dist"], report_count=B_PARAMS["count"],
                                  report_time_s=B_PARAMS["time_s"])


def test_inputs_are_not_vacuous(ctx):
    assert ctx["n_push"] == 80 and len(ctx["segs"]) == 88
    for k in ("vehicle", "time", "lon", "lat", "accuracy"):   # either kind reads back to the same points
        assert ctx["pts"][0][k].tobytes() == ctx["pts"][1][k].tobytes(), k
    assert ctx["pts"][0]["vehicle"].tolist() == ctx["arr"]["vehicle"].tolist()
    for privacy in (1, 2):
        m = ar.Anonymiser(Q, privacy)
        assert m.add(ctx["segs"])["kept"] == 88
        assert m.flush()[1]["rows_kept"] > 0


@pytest.mark.parametrize("privacy", [1, 2])
@pytest.mark.parametrize("gran", ["20s", "one_push"])
@pytest.mark.parametrize("kind", [0, 1])
def test_messages_to_tiles(ctx, kind, gran, privacy):
    assert messages_to_tiles(ctx, kind, gran, privacy) == (80, 8)


def messages_to_tiles(ctx, kind, gran, privacy):
    """Messages -> directory -> sessions -> tile store -> CSV on the GPU against push() fed the host
    reader's arrays, the session model and the anonymiser model; returns the reports forwarded by the
    pushes and by the final punctuate."""
    arr, pts, fmt = ctx["arr"], ctx["pts"][kind], ctx["fmt"][kind]
    cuts = sr.slices(arr, {"20s": 20.0, "one_push": None}[gran])
    # the yardstick: push() fed the host reader's arrays and the model's indices
    plain = _session(ctx)
    want = []
    for a, b in cuts:
        plain.push(pts["vehicle"][a:b], pts["time"][a:b], pts["lon"][a:b], pts["lat"][a:b], pts["accuracy"][a:b],
                   pts["stamp_ms"][a:b])
        want.append((plain.windows().copy(), plain.reports().copy()))
    plain.punctuate(ctx["ts"])
    want.append((plain.windows().copy(), plain.reports().copy()))
    plain.close()
    # the new route
    sess = _session(ctx)
    vdir = engine.VehicleDirectory(ctx["n"])
    store = engine.TileStore(0, Q, privacy, initial_rows=32)
    got = []
    for a, b in cuts:
        out, info = sess.push_messages([msg_text.text(arr, kind, a, b)], fmt, vdir)
        assert info["points"] == b - a and info["dropped"] == 0
        c = store.add_session(sess)
        assert c["kept"] == out["forwarded"] and c["skipped"] == 0
        got.append((sess.windows().copy(), sess.reports().copy()))
    out = sess.punctuate(ctx["ts"])
    store.add_session(sess)
    got.append((sess.windows().copy(), sess.reports().copy()))
    assert len(got) == len(want)
    for (gw, gr), (ww, wr) in zip(got, want):
        assert gw.tobytes() == ww.tobytes() and gr.tobytes() == wr.tobytes()
    # ... which are the session model's
    model = ctx["model"]
    wins, reps, n_win = [], [], 0
    for (gw, gr), (a, _) in zip(got, cuts + [(0, 0)]):
        gw, gr = gw.copy(), gr.copy()
        if len(wins) < len(cuts):
            gw["arrival"] += np.uint32(a)
        gr["window"] += np.uint32(n_win)
        n_win += len(gw)
        wins.append(gw)
        reps.append(gr)
    assert np.concatenate(wins).tobytes() == model.window_array().tobytes()
    assert np.concatenate(reps).tobytes() == model.report_array().tobytes()
    pushed, punctuated = sum(len(r) for _, r in got[:-1]), len(got[-1][1])
    assert pushed == ctx["n_push"] and pushed + punctuated == len(ctx["segs"])
    # the flushed files are the anonymiser model's
    anon = ar.Anonymiser(Q, privacy)
    anon.add(ctx["segs"])
    files, counts = store.flush()
    mfiles, mcounts = anon.flush()
    assert list(files.items()) == list(mfiles.items()) and counts == mcounts and len(files) > 0
    print("stream", kind, gran, privacy, counts, sess.messages_ms())
    store.close()
    vdir.close()
    sess.close()
    return pushed, punctuated


@pytest.mark.parametrize("kind", [0, 1])
def test_stream_cli_writes_the_models_files(ctx, kind, tmp_path):
    """python -m reporter_amd.stream as a child process, in polls of about 64 KiB."""
    privacy = 2
    anon = ar.Anonymiser(Q, privacy)
    anon.add(ctx["segs"])
    mfiles, _ = anon.flush()
    src = tmp_path / "in"
    src.mkdir()
    text = msg_text.text(ctx["arr"], kind)
    half = text.index(b"\n", len(text) // 2) + 1
    (src / "a.txt").write_bytes(text[:half])
    (src / "b.txt").write_bytes(text[half:])
    conf = tmp_path / "conf.json"
    conf.write_text(json.dumps({"meili": {"default": {}}, "reporter_amd": {"graph": ctx["path"]}}))
    out = tmp_path / "out"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "reporter_amd.stream", "--formatter", SPEC[kind], "--match-config", str(conf),
                        "--output-location", str(out), "--privacy", str(privacy), "--quantisation", str(Q),
                        "--flush-interval", "100000", "--max-vehicles", "32", "--poll-bytes", "65536",
                        "--report-dist", str(B_PARAMS["dist"]), "--report-count", str(B_PARAMS["count"]),
                        "--report-time", str(B_PARAMS["time_s"]), str(src)],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    stats = json.loads(r.stdout.strip().splitlines()[-1])
    assert stats["messages"] == 12800 and stats["forwarded"] == 88 and stats["vehicles"] == 32 and stats["polls"] > 5
    written = {}
    for root, _, fs in os.walk(out):
        for f in fs:
            p = os.path.join(root, f)
            written[os.path.relpath(p, out)] = open(p, "rb").read()
    assert written == dict(mfiles) and len(written) > 0
