"""The stream snapshot on the GPU (DESIGN.md §3 rule 15): a stream that is stopped anywhere, saved,
torn down, rebuilt from the blob and continued gives the output of the stream that never stopped --
windows, forwarded reports, final store, directory names and flushed files, bit for bit.

Inputs: those of tests/test_gpu_stream.py (small_world, 32 vehicles x 400 points at 1 Hz, seed 11,
set-B thresholds 1200 m / 20 / 150 s, Q = 60, sr.slices(arr, 20.0): 22 pushes).  The state behind
each cut, from the two CPU models alone (asserted before the GPU is used):

    saved after push   arrivals   vehicles seen / holding   points held   forwarded   trims
    1                       210   20 / 20                            210           0       0
    12                    7,184   32 / 32                          3,217          19      38
    22 (before punctuate) 12,800  32 / 32                          3,602          80      88   (8 more at punctuate)

and, for the arrivals with vehicle % 3 != 1 (8,400 arrivals, 21 vehicles): 2,017 points and 14
forwarded at cut 12, 51 forwarded by the last push, 56 after the punctuate."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import anonymiser_ref as ar
import messages_ref
import msg_text
import snapshot_ref as sn
import stream_ref as sr
from reporter_amd import _lib, engine, graphfile, world

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B_PARAMS = dict(dist=1200.0, count=20, time_s=150.0)
Q = 60
PRIVACY = 2
SPEC = {0: "@sv@,@0@2@3@1@4", 1: "@json@uuid@la@lo@when@acc@yyyy-MM-dd HH:mm:ss"}
DT = (np.uint64, np.uint64, np.float64, np.float64, np.int32, np.int32)
ROWS = {1: (210, 20, 20, 210, 0, 0), 12: (7184, 32, 32, 3217, 19, 38), 22: (12800, 32, 32, 3602, 80, 88)}


def _model_rows(model, pts, cuts, at):
    """The sequential model pushed cut by cut; the table's row behind every cut in `at`."""
    rows = {}
    for k, (a, b) in enumerate(cuts, 1):
        model.push(pts["vehicle"][a:b], pts["time"][a:b], pts["lon"][a:b], pts["lat"][a:b], pts["accuracy"][a:b],
                   pts["stamp_ms"][a:b])
        if k in at:
            rows[k] = (b, len(set(pts["vehicle"][:b].tolist())), sum(1 for v in model.v if len(v)),
                       sum(len(v) for v in model.v), len(model.reports), model.counts["trims"])
    return rows


@pytest.fixture(scope="module")
def ctx(built_lib, small_world):
    g = graphfile.load(small_world)
    tr = world.generate_traces(small_world, n_traces=32, n_points=400, rate_s=1.0, noise_m=5.0, seed=11)
    arr = sr.interleave(tr)
    fmt = msg_text.formats(engine)
    text = msg_text.text(arr, 0)
    pts = engine.parse_messages_host([text], fmt[0], strict=True)
    pts["vehicle"] = messages_ref.Directory(32).assign(messages_ref.parse([text], fmt[0])["point_names"])
    pts["stamp_ms"] = (pts["time"] * 1000.0).astype(np.int64)
    cuts = sr.slices(arr, 20.0)
    ts = int(arr["time"].max() * 1000) + 10 ** 7
    match = sr.oracle_matcher(g, engine.default_options(1))
    model = sr.Sessions(32, match, **B_PARAMS)
    rows = _model_rows(model, pts, cuts, (1, 12, 22))
    model.punctuate(ts)
    segs = [(int(r["id"]), int(r["next_id"]), float(r["t0"]), float(r["t1"]), int(r["length"]), int(r["queue_length"]))
            for r, _, _ in model.reports]
    # the arrivals of two vehicles in three
    keep = pts["vehicle"] % 3 != 1
    hole = {k: pts[k][keep] for k in ("vehicle", "time", "lon", "lat", "accuracy", "stamp_ms")}
    hcuts = sr.slices(hole, 20.0)
    hmodel = sr.Sessions(32, match, **B_PARAMS)
    hrows = _model_rows(hmodel, hole, hcuts, (12, len(hcuts)))
    hpush = len(hmodel.reports)
    hmodel.punctuate(ts)
    # the table, before any GPU work
    assert len(cuts) == 22 and rows == ROWS and len(segs) == 88, (len(cuts), rows, len(segs))
    assert len(hole["vehicle"]) == 8400 and len(set(hole["vehicle"].tolist())) == 21
    assert hrows[12][3:5] == (2017, 14) and hpush == 51 and len(hmodel.reports) == 56, (hrows, hpush, len(hmodel.reports))
    anon = ar.Anonymiser(Q, PRIVACY)
    anon.add(segs)
    mfiles, mcounts = anon.flush()
    eng = engine.Engine(small_world, 0)
    bm = engine.BatchMatcher(eng)
    yield {"arr": arr, "fmt": fmt, "pts": pts, "cuts": cuts, "ts": ts, "model": model, "segs": segs, "hole": hole,
           "hcuts": hcuts, "hmodel": hmodel, "mfiles": mfiles, "mcounts": mcounts, "eng": eng, "bm": bm, "path": small_world,
           "runs": {}}
    bm.close()
    eng.close()


def _session(ctx, nv=32):
    return engine.VehicleSessions(ctx["bm"], nv, report_dist_m=B_PARAMS["dist"], report_count=B_PARAMS["count"],
                                  report_time_s=B_PARAMS["time_s"])


def _objects(ctx, nv=32):
    return _session(ctx, nv), engine.VehicleDirectory(nv), engine.TileStore(0, Q, PRIVACY, initial_rows=32)


def _close(objs):
    for o in reversed(objs):
        o.close()


def _pushes(ctx, kind, objs, first, last, after_push=None):
    """Pushes first + 1 .. last of the stream as messages; the calls' (windows, reports) bytes."""
    sess, vdir, store = objs
    got = []
    for k in range(first, last):
        a, b = ctx["cuts"][k]
        sess.push_messages([msg_text.text(ctx["arr"], kind, a, b)], ctx["fmt"][kind], vdir)
        store.add_session(sess)
        got.append((sess.windows().tobytes(), sess.reports().tobytes()))
        if after_push:
            after_push(k + 1)
    return got


def _finish(ctx, objs):
    """The store after the last push, the punctuate's output, the names and the flush."""
    sess, vdir, store = objs
    st = {k: v.copy() for k, v in sess.store().items()}
    sess.punctuate(ctx["ts"])
    store.add_session(sess)
    last = (sess.windows().tobytes(), sess.reports().tobytes())
    files, counts = store.flush()
    return {"store": st, "last": last, "names": vdir.names(), "files": files, "counts": counts}


def _same_store(a, b):
    """Equal stores, whatever their n_vehicles (the vehicles past the shorter one hold nothing)."""
    n = min(len(a["cnt"]), len(b["cnt"]))
    for k in ("cnt", "max_sep", "last_update"):
        assert a[k][:n].tobytes() == b[k][:n].tobytes(), k
        assert not a[k][n:].any() and not b[k][n:].any(), k
    for k in ("lon", "lat", "time", "accuracy"):
        assert a[k].tobytes() == b[k].tobytes(), k


def _run_a(ctx, kind):
    """The stream that never stops (once per kind)."""
    if kind not in ctx["runs"]:
        objs = _objects(ctx)
        calls = _pushes(ctx, kind, objs, 0, 22)
        end = _finish(ctx, objs)
        _close(objs)
        assert list(end["files"].items()) == list(ctx["mfiles"].items()) and end["counts"] == ctx["mcounts"] and len(end["files"]) > 0
        ctx["runs"][kind] = {"calls": calls, "end": end}
    return ctx["runs"][kind]


def _same_end(ctx, got, want):
    _same_store(got["store"], want["store"])
    assert got["last"] == want["last"]
    assert got["names"] == want["names"]
    assert list(got["files"].items()) == list(want["files"].items()) and got["counts"] == want["counts"]
    assert list(got["files"].items()) == list(ctx["mfiles"].items()) and got["counts"] == ctx["mcounts"]


@pytest.mark.parametrize("cut", [0, 1, 12, 22])
@pytest.mark.parametrize("kind", [0, 1])
def test_stopped_equals_unbroken(ctx, kind, cut, monkeypatch):
    a = _run_a(ctx, kind)
    objs = _objects(ctx)
    head = _pushes(ctx, kind, objs, 0, cut)
    assert head == a["calls"][:cut]
    blob = engine.save_stream(*objs, user=b"cut %d" % cut)
    _close(objs)
    info = engine.snapshot_info(blob)
    if cut:
        assert (info["names"], info["vehicles"], info["points"]) == ROWS[cut][1:4]
    assert info["user"] == b"cut %d" % cut and info["quantisation"] == Q
    if kind == 0 and cut == 1:
        monkeypatch.setenv("RM_LINES_HASH_BITS", "4")   # the loading side alone: the table is rebuilt under its own mask
    objs = _objects(ctx, 48 if cut == 12 else 32)
    got = engine.load_stream(blob, *objs)
    assert (got["names"], got["vehicles"], got["points"], got["rows"]) == (info["names"], info["vehicles"], info["points"], info["rows"])
    assert len(objs[0].reports()) == 0 and len(objs[0].windows()) == 0
    assert objs[2].add_session(objs[0]) == dict(kept=0, skipped=0, rows=0, held=info["rows"])
    assert objs[1].size == info["names"]
    tail = _pushes(ctx, kind, objs, cut, 22)
    assert len(tail) == 22 - cut
    for k, (g, w) in enumerate(zip(tail, a["calls"][cut:])):
        assert g == w, "call %d after the cut" % (k + 1)
    end = _finish(ctx, objs)
    _close(objs)
    _same_end(ctx, end, a["end"])
    print("snapshot", kind, cut, len(blob), got["ms"], engine.save_stream.last["ms"])


def test_save_is_read_only_and_canonical(ctx):
    a = _run_a(ctx, 0)
    objs = _objects(ctx)
    sess, vdir, store = objs
    blobs, calls = {}, []
    for k, (lo, hi) in enumerate(ctx["cuts"], 1):
        sess.push_messages([msg_text.text(ctx["arr"], 0, lo, hi)], ctx["fmt"][0], vdir)
        before = (sess.windows().tobytes(), sess.reports().tobytes())
        early = engine.save_stream(*objs, user=b"early")   # between the push and add_session: the call's read-outs stay
        assert (sess.windows().tobytes(), sess.reports().tobytes()) == before
        added = store.add_session(sess)
        assert added["kept"] == len(sess.reports())
        blobs[k] = engine.save_stream(*objs, user=b"u")
        assert (sess.windows().tobytes(), sess.reports().tobytes()) == before
        assert engine.snapshot_info(early)["points"] == engine.snapshot_info(blobs[k])["points"]
        calls.append(before)
    assert calls == a["calls"]
    end = _finish(ctx, objs)
    _close(objs)
    _same_end(ctx, end, a["end"])
    # save -> load -> save gives the same bytes; snapshot_info reports the table's numbers
    blob = blobs[12]
    objs = _objects(ctx)
    engine.load_stream(blob, *objs)
    again = engine.save_stream(*objs, user=b"u")
    _close(objs)
    assert again == blob
    for k in range(3):   # a closed object is an error, not an absent one
        part = [o if j == k else None for j, o in enumerate(objs)]
        with pytest.raises(_lib.RmError, match="closed"):
            engine.save_stream(*part)
        with pytest.raises(_lib.RmError, match="closed"):
            engine.load_stream(blob, *part)
    secs, table = sn.read(blob)
    info = engine.snapshot_info(blob)
    count = {e[0]: e[4] for e in table}
    assert info["names"] == count[sn.DIR_OFF] - 1 == 32 and info["vehicles"] == count[sn.SESS_REC] == 32
    assert info["points"] == count[sn.SESS_TIME] == count[sn.SESS_LON] == 3217 and info["rows"] == count[sn.TILE_ROWS]
    assert info["bytes"] == len(blob) and info["user"] == b"u" == secs[sn.USER]
    assert all(sn.checksum(secs[e[0]]) == e[5] and e[2] % 16 == 0 for e in table)
    rec = np.frombuffer(secs[sn.SESS_REC], sn.REC_DTYPE)
    assert rec["vehicle"].tolist() == list(range(32)) and int(rec["cnt"].sum()) == 3217
    assert np.frombuffer(secs[sn.TILE_META], sn.META_DTYPE)["arrivals"][0] == 19


def test_holes(ctx):
    """Sessions alone, a third of the vehicles never seen: the array push, cut at 12."""
    h, cuts = ctx["hole"], ctx["hcuts"]

    def pushes(sess, first, last):
        got = []
        for a, b in cuts[first:last]:
            sess.push(h["vehicle"][a:b], h["time"][a:b], h["lon"][a:b], h["lat"][a:b], h["accuracy"][a:b], h["stamp_ms"][a:b])
            got.append((sess.windows().tobytes(), sess.reports().copy()))
        return got

    def finish(sess):
        st = {k: v.copy() for k, v in sess.store().items()}
        sess.punctuate(ctx["ts"])
        return st, sess.windows().tobytes(), sess.reports().copy()

    sess = _session(ctx)
    want = pushes(sess, 0, len(cuts))
    want_end = finish(sess)
    sess.close()
    sess = _session(ctx)
    head = pushes(sess, 0, 12)
    blob = engine.save_stream(sessions=sess)
    sess.close()
    info = engine.snapshot_info(blob)
    assert (info["names"], info["vehicles"], info["points"], info["rows"]) == (0, 21, 2017, 0)
    assert sum(len(r) for _, r in head) == 14
    sess = _session(ctx, 40)
    engine.load_stream(blob, sessions=sess)
    tail = pushes(sess, 12, len(cuts))
    end = finish(sess)
    sess.close()
    for (gw, gr), (ww, wr) in zip(head + tail, want):
        assert gw == ww and gr.tobytes() == wr.tobytes()
    _same_store(end[0], want_end[0])
    assert end[1] == want_end[1] and end[2].tobytes() == want_end[2].tobytes()
    # ... which is the sequential model's
    reps = np.concatenate([r for _, r in head + tail] + [end[2]])
    assert sum(len(r) for _, r in head + tail) == 51 and len(reps) == 56
    mreps = ctx["hmodel"].report_array()
    for f in ("id", "next_id", "t0", "t1", "length", "queue_length"):
        assert reps[f].tobytes() == mreps[f].tobytes(), f
    assert reps["vehicle"].tolist() == mreps["vehicle"].tolist()


def _arrays(segs):
    return [np.array([s[k] for s in segs], dt) for k, dt in enumerate(DT)]


def test_tile_store_alone(ctx):
    segs = ctx["segs"]
    store = engine.TileStore(0, Q, PRIVACY, initial_rows=32)
    store.add(*_arrays(segs[:44]))
    blob = engine.save_stream(store=store)
    store.close()
    other = engine.TileStore(0, 120, PRIVACY, initial_rows=32)
    with pytest.raises(_lib.RmError, match="quantisation"):
        engine.load_stream(blob, store=other)
    model = ar.Anonymiser(120, PRIVACY)
    assert other.add(*_arrays(segs)) == model.add(segs)   # ... and then works as ever
    files, counts = other.flush()
    mfiles, mcounts = model.flush()
    assert list(files.items()) == list(mfiles.items()) and counts == mcounts
    other.close()
    store = engine.TileStore(0, Q, PRIVACY, initial_rows=4)
    got = engine.load_stream(blob, store=store)
    assert got["rows"] == engine.snapshot_info(blob)["rows"] > 0
    store.add(*_arrays(segs[44:]))
    files, counts = store.flush()
    store.close()
    assert list(files.items()) == list(ctx["mfiles"].items()) and counts == ctx["mcounts"]


def _refused_as_host(blob, *objs, **kw):
    """The load fails with the message the host check gives for the same blob."""
    with pytest.raises(_lib.RmError) as host:
        engine.snapshot_info(blob)
    with pytest.raises(_lib.RmError) as dev:
        engine.load_stream(blob, *objs, **kw)
    assert str(dev.value) == str(host.value), (str(dev.value), str(host.value))
    return str(dev.value)


def _flip(blob, kind, bit=13):
    _, table = sn.read(blob)
    off = next(e[2] for e in table if e[0] == kind)
    b = bytearray(blob)
    b[off + bit // 8] ^= 1 << (bit % 8)
    return bytes(b)


def test_refusals_leave_everything_usable(ctx):
    a = _run_a(ctx, 0)
    # the blobs behind pushes 1 and 12
    objs = _objects(ctx)
    blobs = {}
    _pushes(ctx, 0, objs, 0, 12, after_push=lambda k: blobs.__setitem__(k, engine.save_stream(*objs)) if k in (1, 12) else None)
    # a load into objects that hold something: refused, and they go on as if nothing had been tried
    with pytest.raises(_lib.RmError, match="not empty"):
        engine.load_stream(blobs[1], *objs)
    for k in range(3):   # each alone, the others empty
        part = [o if j == k else None for j, o in enumerate(objs)]
        with pytest.raises(_lib.RmError, match="not empty"):
            engine.load_stream(blobs[12], *part)
    tail = _pushes(ctx, 0, objs, 12, 22)
    assert tail == a["calls"][12:]
    _same_end(ctx, _finish(ctx, objs), a["end"])
    _close(objs)
    # targets too small
    small = _session(ctx, 16)
    with pytest.raises(_lib.RmError, match="n_vehicles"):
        engine.load_stream(blobs[12], sessions=small)
    assert not small.store()["cnt"].any() and len(small.store()["lon"]) == 0
    small.close()
    vdir = engine.VehicleDirectory(16)
    with pytest.raises(_lib.RmError, match="max_vehicles"):
        engine.load_stream(blobs[1], directory=vdir)
    assert vdir.size == 0
    vdir.close()
    # damaged and forged blobs into one set of objects, which stay empty and usable throughout
    objs = _objects(ctx)
    assert _refused_as_host(_flip(blobs[12], sn.SESS_LON), *objs) == "snapshot: a section's checksum does not match"
    assert _refused_as_host(_flip(blobs[12], sn.TILE_ROWS), *objs) == "snapshot: a section's checksum does not match"
    secs, _ = sn.read(blobs[12])
    rec = np.frombuffer(secs[sn.SESS_REC], sn.REC_DTYPE).copy()
    rec["cnt"][3] += 1
    forged = sn.write({**secs, sn.SESS_REC: rec.tobytes()})
    assert _refused_as_host(forged, *objs) == "snapshot: the session records' cnt do not add up to the point count"
    rec = np.frombuffer(secs[sn.SESS_REC], sn.REC_DTYPE).copy()
    rec["vehicle"][[5, 6]] = rec["vehicle"][[6, 5]]
    forged = sn.write({**secs, sn.SESS_REC: rec.tobytes()})
    assert _refused_as_host(forged, *objs) == "snapshot: session vehicle indices are not strictly increasing"
    off = np.frombuffer(secs[sn.DIR_OFF], "<u8").copy()
    off[-1] += 8
    forged = sn.write({**secs, sn.DIR_OFF: off.tobytes()})
    assert _refused_as_host(forged, *objs) == "snapshot: name offsets do not stay inside the name bytes"
    # two equal names show only as the table is rebuilt: the directory is emptied again
    names = secs[sn.DIR_BYTES]
    off = np.frombuffer(secs[sn.DIR_OFF], "<u8")
    each = [names[int(off[k]):int(off[k + 1])] for k in range(len(off) - 1)]
    each[7] = each[0]
    forged = sn.write({**secs, sn.DIR_BYTES: b"".join(each),
                       sn.DIR_OFF: np.cumsum([0] + [len(x) for x in each]).astype("<u8").tobytes()})
    assert _refused_as_host(forged, *objs) == "snapshot: two names are equal"
    assert objs[1].size == 0 and objs[2].flush()[1]["rows_in"] == 0 and not objs[0].store()["cnt"].any()
    calls = _pushes(ctx, 0, objs, 0, 22)
    assert calls == a["calls"]
    _same_end(ctx, _finish(ctx, objs), a["end"])
    _close(objs)


def _tree(d):
    out = {}
    for root, _, fs in os.walk(d):
        for f in fs:
            p = os.path.join(root, f)
            out[os.path.relpath(p, d)] = open(p, "rb").read()
    return out


def test_cli_stop_and_resume(ctx, tmp_path):
    src = tmp_path / "in"
    src.mkdir()
    text = msg_text.text(ctx["arr"], 0)
    half = text.index(b"\n", len(text) // 2) + 1
    (src / "a.txt").write_bytes(text[:half])
    (src / "b.txt").write_bytes(text[half:])
    conf = tmp_path / "conf.json"
    conf.write_text(json.dumps({"meili": {"default": {}}, "reporter_amd": {"graph": ctx["path"]}}))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def child(out, *more):
        return subprocess.run([sys.executable, "-m", "reporter_amd.stream", "--formatter", SPEC[0], "--match-config", str(conf),
                               "--output-location", str(out), "--privacy", str(PRIVACY), "--quantisation", str(Q),
                               "--flush-interval", "100", "--max-vehicles", "32", "--poll-bytes", "65536",
                               "--report-dist", str(B_PARAMS["dist"]), "--report-count", str(B_PARAMS["count"]),
                               "--report-time", str(B_PARAMS["time_s"]), *more, str(src)],
                              capture_output=True, text=True, timeout=300, env=env)

    stats = lambda r: json.loads(r.stdout.strip().splitlines()[-1])
    r = child(tmp_path / "whole")
    assert r.returncode == 0, r.stdout + r.stderr
    whole = stats(r)
    assert whole["messages"] == 12800 and whole["forwarded"] == 88 and whole["vehicles"] == 32 and whole["flushes"] > 2
    ck = str(tmp_path / "ck")
    r = child(tmp_path / "parts", "--checkpoint", ck, "--stop-after-polls", "3")
    assert r.returncode == 0, r.stdout + r.stderr
    first = stats(r)
    assert first["polls"] == 3 and first.get("stopped") and 0 < first["messages"] < 12800
    user = json.loads(engine.snapshot_info(open(ck, "rb").read())["user"].decode())
    assert user["stats"]["polls"] == 3 and [os.path.basename(p) for p, _ in user["inputs"]] == ["a.txt", "b.txt"]
    r = child(tmp_path / "parts", "--checkpoint", ck, "--resume")
    assert r.returncode == 0, r.stdout + r.stderr
    assert stats(r) == whole
    assert _tree(tmp_path / "parts") == _tree(tmp_path / "whole") and len(_tree(tmp_path / "whole")) > 0
    # another input than the checkpoint's: refused
    # the checkpoint behind the final flush says so: a resume of a finished stream does nothing
    assert json.loads(engine.snapshot_info(open(ck, "rb").read())["user"].decode())["done"] is True
    r = child(tmp_path / "parts", "--checkpoint", ck, "--resume")
    assert r.returncode == 0, r.stdout + r.stderr
    assert stats(r) == whole and _tree(tmp_path / "parts") == _tree(tmp_path / "whole")
    (src / "b.txt").write_bytes(text[half:] + text[half:text.index(b"\n", half) + 1])
    r = child(tmp_path / "parts2", "--checkpoint", ck, "--resume")
    assert r.returncode != 0 and "other inputs" in r.stderr
    assert not os.path.exists(tmp_path / "parts2") or not _tree(tmp_path / "parts2")
