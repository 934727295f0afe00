"""Date patterns read on the GPU (DESIGN.md §3 rule 18; lines.hip k_line_parse<KIND, true>):

  * the device reader against the host generic reader, for eight patterns and both kinds of line,
    over the first 2,000 arrivals of test_gpu_stream.py's small case (32 vehicles at 1 Hz, seed 11)
    with valid lines outside the compact layout and malformed times mixed in; the clean text must be
    read by the device alone and give back the instants that were written;
  * lines at the edges of the reader's 4096-byte windows;
  * the stream, unsharded and on two ranks, written with epoch seconds and under two patterns: the
    same windows, reports and tile files byte for byte;
  * a checkpoint written under a pattern, resumed in a fresh process whose registry numbers the
    pattern differently.

tests/test_time_pattern_host.py pins the host generic reader to the plain-Python restatement."""
import hashlib
import json
import os
import random
import subprocess
import sys
import time as _time

import numpy as np
import pytest

import msg_text
import stream_ref as sr
import time_pattern_ref as ref
from reporter_amd import engine, world

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B_PARAMS = dict(report_dist_m=1200.0, report_count=20, report_time_s=150.0)
Q = 60
PATTERNS = ["yyyy-MM-dd'T'HH:mm:ssZZ", "yyyy-MM-dd'T'HH:mm:ss.SSSZZ", "yyyyMMddHHmmss", "dd/MMM/yyyy HH:mm:ss",
            "M/d/yy h:mm:ss a", "yyyy-DDD'T'kk:mm:ssZ", "d MMMM yyyy HH:mm:ss.SSSSSS", "yyyy-MM-dd KK:mm:ss a"]
ISO_MS = "yyyy-MM-dd'T'HH:mm:ss.SSSZZ"
DIGITS = "yyyyMMddHHmmss"


def _fields(t, off_min=0, ms=0):
    """The instant t (epoch seconds) as the civil time of a clock off_min minutes ahead of UTC."""
    g = _time.gmtime(int(t) + 60 * off_min)
    return ref.fields(g[0], g[1], g[2], g[3], g[4], g[5], ms, off_min)


def _format(kind, pattern):
    line = engine.LineFormat(time_pattern=pattern) if pattern else engine.LineFormat()
    return engine.MessageFormat(kind, line, msg_text.KEYS)


def _message(arr, j, kind, tm, odd=False):
    """msg_text.message with the time text `tm` (None: epoch seconds)."""
    name = msg_text.name(int(arr["vehicle"][j]))
    lon, lat, acc = (str(np.float32(arr[k][j])) for k in ("lon", "lat", "accuracy"))
    if tm is None:
        tm, quoted = "%d" % int(arr["time"][j]), "%d" % int(arr["time"][j])
    else:
        quoted = '"%s"' % tm
    if kind == 0:
        return (" %s , %s,%s,\t%s,%s \r" if odd else "%s,%s,%s,%s,%s") % (name, tm, lat, lon, acc)
    if odd:
        return ' {"lo" : %s , "acc":"%s","when":%s, "uuid":"%s","la":%s}\t' % (lon, acc, quoted, name, lat)
    return '{"uuid":"%s","when":%s,"la":%s,"lo":%s,"acc":%s,"speed":12.5}' % (name, quoted, lat, lon, acc)


def _text(arr, kind, pattern, a, b, off_min=0, rng=None):
    """Arrivals [a, b) as text under `pattern`: the canonical spelling, or with rng any spelling the
    rule reads."""
    out = []
    for j in range(a, b):
        tm = None if pattern is None else ref.render(pattern, _fields(arr["time"][j], off_min, (j * 37) % 1000), rng)
        out.append(_message(arr, j, kind, tm))
    return ("\n".join(out) + "\n").encode() if out else b""


@pytest.fixture(scope="module")
def ctx(built_lib, small_world):
    tr = world.generate_traces(small_world, n_traces=32, n_points=400, rate_s=1.0, noise_m=5.0, seed=11)
    arr = sr.interleave(tr)
    eng = engine.Engine(small_world, 0)
    bm = engine.BatchMatcher(eng)
    yield {"arr": arr, "eng": eng, "bm": bm, "path": small_world, "ts": int(arr["time"].max() * 1000) + 10 ** 7}
    bm.close()
    eng.close()


def _same_points(got, want):
    for k in ("uuid", "time", "lon", "lat", "accuracy"):
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k


COUNTS = ("lines", "blank", "outside", "points", "vehicles", "dropped")


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("p", range(len(PATTERNS)))
def test_device_reader_equals_host_reader(ctx, p, kind):
    pattern, arr, bm = PATTERNS[p], ctx["arr"], ctx["bm"]
    fmt = _format(kind, pattern)
    n = 2000
    rng = random.Random(100 + 2 * p + kind)
    # ---- the clean text: any spelling the rule reads, every line in the compact layout
    offs = [rng.choice([0, 0, 480, -210, 1439, -1439]) if "Z" in pattern else 0 for _ in range(n)]
    clean = [_message(arr, j, kind, ref.render(pattern, _fields(arr["time"][j], offs[j], (j * 37) % 1000), rng)) for j in range(n)]
    chunks = [("\n".join(clean[:700]) + "\n").encode(), ("\n".join(clean[700:])).encode()]   # no final newline
    host = engine.parse_messages_host(chunks, fmt, strict=True)
    assert host["time"].tolist() == arr["time"][:n].tolist()        # the instants that were written
    if kind == 0:
        _same_points(bm.parse_lines(chunks, fmt.line), host)
        assert bm.lines_info()["host_lines"] == 0 and bm.vehicle_names(chunks) == host["names"]
    sess = engine.VehicleSessions(bm, 32, **B_PARAMS)
    vdir = engine.VehicleDirectory(32)
    out, info = sess.push_messages(chunks, fmt, vdir)
    _same_points(bm.line_points(), host)
    assert info == dict(lines=n, blank=0, outside=0, points=n, vehicles=32, host_lines=0, ids_on_host=0, dropped=0)
    assert vdir.names() == host["names"]
    print("pattern", pattern, "kind", kind, sess.messages_ms())
    vdir.close()
    sess.close()
    # ---- mixed: valid lines outside the compact layout, spoiled times, a number where JSON wants a string
    lines, n_odd, n_spoiled = [], 0, 0
    for j in range(n):
        f = _fields(arr["time"][j], offs[j], (j * 37) % 1000)
        if j % 10 == 9:
            lines.append(_message(arr, j, kind, ref.render(pattern, f, rng), odd=True))
            n_odd += 1
        elif j % 7 == 3:
            tm = ref.mutate(pattern, f, ref.MUTATIONS[(j // 7) % 8], rng)
            v = ref.parse(pattern, tm)
            if v is not None and v != arr["time"][j]:
                tm = ref.render(pattern, f, rng)   # (read, but to another instant: held to the host on the CPU)
            n_spoiled += v is None
            lines.append(_message(arr, j, kind, tm))
        else:
            lines.append(clean[j])
        if j % 400 == 5:
            lines.append("")
        if kind == 1 and j % 500 == 6:
            lines.append(_message(arr, j, kind, None))
    assert n_spoiled > 100
    chunks = [("\n".join(lines[:900]) + "\n").encode(), b"", ("\n".join(lines[900:]) + "\n").encode()]
    host = engine.parse_messages_host(chunks, fmt)
    assert host["info"]["dropped"] >= n_spoiled - 40 and host["info"]["points"] > 1500 and host["info"]["blank"] == 5
    sess = engine.VehicleSessions(bm, 32, **B_PARAMS)
    vdir = engine.VehicleDirectory(32)
    out, info = sess.push_messages(chunks, fmt, vdir)
    _same_points(bm.line_points(), host)
    assert {k: info[k] for k in COUNTS} == {k: host["info"][k] for k in COUNTS}
    assert info["host_lines"] >= n_odd + info["dropped"] and info["ids_on_host"] == 0
    assert sess.dropped_messages() == host["dropped"] and len(host["dropped"]) == 64
    assert all(why == "malformed time (%s)" % pattern for _, _, why in host["dropped"])
    assert vdir.names() == host["names"]
    vdir.close()
    sess.close()


def _line(n, veh, t, tm):
    """A compact line of exactly n bytes with its newline (the id padded), the time text tm."""
    tail = ",%s,47.%06d,8.%06d,%02d\n" % (tm, t % 1000000, (7 * t) % 1000000, t % 50)
    uid = "w%d" % veh
    assert n >= len(uid) + len(tail)
    return (uid + "p" * (n - len(uid) - len(tail)) + tail).encode()


def test_window_edges(ctx):
    pattern = "yyyy-MM-dd'T'HH:mm:ssZZ"
    fmt = engine.LineFormat(time_pattern=pattern)
    t0 = 1483250740
    long_tm = lambda t: ref.render(pattern, _fields(t, 480))            # 25 bytes
    short_tm = lambda t: ref.render(pattern, _fields(t, 0)).replace("+00:00", "Z")   # 20 bytes
    # a 100-byte line, then 64-byte lines that start 36 bytes into each 64: bytes 4096 and 8192 fall
    # inside a time field (a 64-byte line's time is its bytes [16, 41))
    text = _line(100, 0, t0, long_tm(t0)) + b"".join(_line(64, k % 7, t0 + 1 + k, long_tm(t0 + 1 + k)) for k in range(140))
    for edge in (4096, 8192):
        start = text.rfind(b"\n", 0, edge) + 1
        assert edge - start == 28 and text[start + 16:start + 41] == long_tm(t0 + 1 + (start - 100) // 64).encode()
    text += b"".join(("a,%s,2,3,4\n" % short_tm(t0 + 200 + k)).encode() for k in range(300))   # 29 bytes: 141 in a window
    assert len("a,%s,2,3,4\n" % short_tm(t0)) == 29
    text += _line(256, 1, t0 + 600, long_tm(t0 + 600)) + _line(257, 2, t0 + 601, long_tm(t0 + 601))
    text += _line(70, 2, t0 + 602, long_tm(t0 + 602)).rstrip(b"\n")                            # no final newline
    assert 4 * 4096 < len(text) <= 5 * 4096
    bm = ctx["bm"]
    cut1 = text.index(b"\n", 4000) + 1
    cut2 = text.index(b"\n", 9000) + 1
    for chunks in ([text], [text[:cut1], text[cut1:cut2], text[cut2:]]):
        want = engine.parse_lines_host(chunks, fmt)
        got = bm.parse_lines(chunks, fmt)
        _same_points(got, want)
        info = bm.lines_info()
        counts = ("lines", "blank", "outside", "points", "vehicles")
        assert {k: info[k] for k in counts} == {k: want["info"][k] for k in counts}
        assert bm.vehicle_names(chunks) == want["names"]
        assert info["points"] == 141 + 300 + 2 + 1
        assert info["host_lines"] == 1 and info["ids_on_host"] == 0   # the 257-byte line alone
        assert got["time"].tolist() == [float(t0 + k) for k in range(141)] + [float(t0 + 200 + k) for k in range(300)] + [
            float(t0 + 600 + k) for k in range(3)]


# ---------------------------------------------------------------- the stream under three spellings
SPELLINGS = [(None, 0), (ISO_MS, 480), (DIGITS, 0)]


def _unsharded(ctx, kind, pattern, off_min, cuts, first=0, objs=None, stop=None):
    """Pushes first .. stop of the stream; without `stop`, to the end with the punctuate and the flush."""
    arr = ctx["arr"]
    fmt = _format(kind, pattern)
    sess, vdir, store = objs or (engine.VehicleSessions(ctx["bm"], 32, **B_PARAMS), engine.VehicleDirectory(32),
                                 engine.TileStore(0, Q, 2, initial_rows=32))
    calls = []
    for a, b in cuts[first:stop]:
        out, info = sess.push_messages([_text(arr, kind, pattern, a, b, off_min)], fmt, vdir)
        assert info["points"] == b - a and info["dropped"] == 0 and info["host_lines"] == 0
        store.add_session(sess)
        calls.append((sess.windows().tobytes(), sess.reports().tobytes()))
    if stop is not None:
        return calls, (sess, vdir, store)
    sess.punctuate(ctx["ts"])
    store.add_session(sess)
    calls.append((sess.windows().tobytes(), sess.reports().tobytes()))
    files, counts = store.flush()
    names = vdir.names()
    for o in (store, vdir, sess):
        o.close()
    return {"calls": calls, "files": list(files.items()), "counts": counts, "names": names}


def _sharded(ctx, kind, pattern, off_min, cuts, R=2):
    arr = ctx["arr"]
    fmt = _format(kind, pattern)
    bms = [engine.BatchMatcher(ctx["eng"]) for _ in range(R)]
    sess = [engine.VehicleSessions(bm, 32, **B_PARAMS) for bm in bms]
    dirs = [engine.VehicleDirectory(32) for _ in range(R)]
    stores = [engine.TileStore(0, Q, 2, initial_rows=8) for _ in range(R)]
    calls = []
    try:
        for a, b in cuts:
            text = _text(arr, kind, pattern, a, b, off_min)
            for r in range(R):
                out, info = sess[r].push_messages([text], fmt, dirs[r], shard=(r, R))
                assert info["points"] == b - a and info["dropped"] == 0 and info["host_lines"] == 0
                stores[r].add_session(sess[r])
                calls.append((sess[r].windows().tobytes(), sess[r].reports().tobytes()))
        for r in range(R):
            sess[r].punctuate(ctx["ts"])
            stores[r].add_session(sess[r])
            calls.append((sess[r].windows().tobytes(), sess[r].reports().tobytes()))
        blobs = [s.export_rows() for s in stores]
        exch = [s.import_owned(blobs, r, R) for r, s in enumerate(stores)]
        files = [list(s.flush()[0].items()) for s in stores]
        return {"calls": calls, "files": files, "exchange": exch, "names": [d.names() for d in dirs]}
    finally:
        for x in stores + dirs + sess + bms:
            x.close()


@pytest.mark.parametrize("kind", [0, 1])
def test_the_stream_does_not_depend_on_the_spelling(ctx, kind):
    cuts = sr.slices(ctx["arr"], 60.0)
    assert 5 <= len(cuts) <= 10
    one = [_unsharded(ctx, kind, p, off, cuts) for p, off in SPELLINGS]
    assert len(one[0]["files"]) > 0 and sum(len(r) for _, r in one[0]["calls"]) > 0 and one[0]["counts"]["rows_kept"] > 0
    assert one[1] == one[0] and one[2] == one[0]
    two = [_sharded(ctx, kind, p, off, cuts) for p, off in SPELLINGS]
    assert all(len(f) > 0 for f in two[0]["files"]) and sum(len(r) for _, r in two[0]["calls"]) > 0
    assert two[1] == two[0] and two[2] == two[0]
    union = dict(f for per_rank in two[0]["files"] for f in per_rank)
    assert union == dict(one[0]["files"])


CHILD = r"""
import hashlib, json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
from reporter_amd import engine
import test_gpu_time_patterns as t
d = json.load(open(sys.argv[3]))
for k in range(5):   # this process numbers its patterns otherwise than the one that saved
    engine.time_pattern_id("yyyy-MM-dd'%d'" % k)
assert engine.time_pattern_id(d["pattern"]) == 16 + 5
eng = engine.Engine(d["graph"], 0)
bm = engine.BatchMatcher(eng)
objs = (engine.VehicleSessions(bm, 32, **t.B_PARAMS), engine.VehicleDirectory(32), engine.TileStore(0, t.Q, 2, initial_rows=32))
engine.load_stream(open(d["blob"], "rb").read(), *objs)
sess, vdir, store = objs
fmt = t._format(d["kind"], d["pattern"])
h = hashlib.sha256()
for path in d["texts"]:
    out, info = sess.push_messages([open(path, "rb").read()], fmt, vdir)
    assert info["dropped"] == 0 and info["host_lines"] == 0
    store.add_session(sess)
    h.update(sess.windows().tobytes()); h.update(sess.reports().tobytes())
sess.punctuate(d["ts"])
store.add_session(sess)
h.update(sess.windows().tobytes()); h.update(sess.reports().tobytes())
files, counts = store.flush()
for name, body in files.items():
    h.update(name.encode()); h.update(body)
h.update(json.dumps(vdir.names()).encode())
print("RESUMED", h.hexdigest(), len(files))
for o in (store, vdir, sess, bm, eng):
    o.close()
"""


def test_a_checkpoint_resumes_in_a_fresh_process(ctx, tmp_path):
    kind, pattern, off = 1, ISO_MS, 480
    cuts = sr.slices(ctx["arr"], 60.0)
    stop = 3
    want = _unsharded(ctx, kind, pattern, off, cuts)
    head, objs = _unsharded(ctx, kind, pattern, off, cuts, stop=stop)
    assert head == want["calls"][:stop]
    blob = engine.save_stream(*objs)
    for o in reversed(objs):
        o.close()
    assert pattern.encode() not in blob   # the format is the loading process's: no pattern, no id in the snapshot
    h = hashlib.sha256()
    for w, r in want["calls"][stop:]:
        h.update(w); h.update(r)
    for name, body in want["files"]:
        h.update(name.encode()); h.update(body)
    h.update(json.dumps(want["names"]).encode())
    texts = []
    for k, (a, b) in enumerate(cuts[stop:]):
        p = tmp_path / ("push%02d.txt" % k)
        p.write_bytes(_text(ctx["arr"], kind, pattern, a, b, off))
        texts.append(str(p))
    (tmp_path / "blob").write_bytes(blob)
    (tmp_path / "job.json").write_text(json.dumps({"pattern": pattern, "kind": kind, "graph": ctx["path"], "ts": ctx["ts"],
                                                   "blob": str(tmp_path / "blob"), "texts": texts}))
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, os.path.join(ROOT, "tests"), str(tmp_path / "job.json")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "RESUMED %s %d" % (h.hexdigest(), len(want["files"])) in r.stdout, r.stdout + r.stderr
