"""Trace-file text parsed and grouped on the GPU (rm_runner_run_lines / rm_runner_parse_lines,
DESIGN.md rule 11) against today's path (read_trace_files + dense_ids + run_points) and against the
generic host reader (rm_lines_parse_host), which tests/test_lines_host.py pins to plain Python."""
import json

import numpy as np
import pytest

from reporter_amd import batch, engine
from test_gpu_stages import _stream

pytestmark = pytest.mark.gpu


def _text_lines(pts):
    return ["v%d,%d,%.6f,%.6f,%d\n" % (u, int(t), la, lo, int(a))
            for u, t, la, lo, a in zip(pts["uuid"], pts["time"], pts["lat"], pts["lon"], pts["accuracy"])]


def _outputs(bm):
    """Everything a run leaves that the batch pipeline reads."""
    so, segs = bm.segments()
    ro, reps, stats = bm.reports()
    fields = [f for f in reps.dtype.names if f != "pad"]
    return dict(trace_uuid=bm.trace_uuid().tobytes(), batch={k: v.tobytes() for k, v in bm.batch().items()},
                seg_off=so.tobytes(), segs=segs.tobytes(), rep_off=ro.tobytes(), reps=[reps[f].tobytes() for f in fields],
                stats=stats.tobytes(), tiles1=bm.tiles(privacy=1), tiles2=bm.tiles(privacy=2))


@pytest.fixture(scope="module")
def stream_case(small_world, tmp_path_factory):
    return make_stream_case(small_world, tmp_path_factory.mktemp("lines"))


def make_stream_case(path, d):
    """_stream's 40 vehicles on the graph at `path` as text in three chunks (files in directory d), and
    what today's path makes of that text."""
    lines = _text_lines(_stream(path))
    a, b = len(lines) // 3, 2 * len(lines) // 3
    chunks = ["".join(lines[:a]).encode(), "".join(lines[a:b]).encode(), "".join(lines[b:]).encode().rstrip(b"\n")]
    paths = []
    for k, c in enumerate(chunks):
        p = d / ("%03d" % k)
        p.write_bytes(c)
        paths.append(str(p))
    uuids, pts = batch.read_trace_files(paths)
    idx, names = batch.dense_ids(uuids)
    eng = engine.Engine(path, 0)
    bm = engine.BatchMatcher(eng)
    bm.run_points(idx, pts["time"], pts["lon"], pts["lat"], pts["accuracy"], inactivity=120, n_uuids=len(names))
    want = _outputs(bm)
    assert bm.sizes()["traces"] == 80 and len(idx) > 19000
    bm.close()
    eng.close()
    return dict(chunks=chunks, names=names, idx=idx, pts=pts, want=want)


def _same_points(got, ref):
    for k in ("uuid", "time", "lon", "lat", "accuracy"):
        assert got[k].dtype == ref[k].dtype and got[k].tobytes() == ref[k].tobytes(), k


def test_run_lines_equals_run_points(small_world, stream_case):
    run_lines_equals_run_points(small_world, stream_case)


def run_lines_equals_run_points(path, c):
    eng = engine.Engine(path, 0)
    bm = engine.BatchMatcher(eng)
    bm.run_lines(c["chunks"], inactivity=120)
    info = bm.lines_info()
    assert info["host_lines"] == 0 and info["ids_on_host"] == 0   # the device readers did the work
    assert info["points"] == len(c["idx"]) == info["lines"] and info["vehicles"] == 40
    assert bm.vehicle_names(c["chunks"]) == c["names"]
    lp = bm.line_points()
    np.testing.assert_array_equal(lp["uuid"], c["idx"])
    np.testing.assert_array_equal(lp["time"], c["pts"]["time"])
    np.testing.assert_array_equal(lp["lon"], c["pts"]["lon"].astype(np.float32))
    np.testing.assert_array_equal(lp["lat"], c["pts"]["lat"].astype(np.float32))
    np.testing.assert_array_equal(lp["accuracy"], c["pts"]["accuracy"])
    assert _outputs(bm) == c["want"]
    ms = bm.lines_ms()
    assert set(ms) == {"upload", "parse", "ids", "windows"} and all(v >= 0 for v in ms.values()) and ms["parse"] > 0
    bm.close()
    eng.close()


def _line(n, veh, t):
    """A compact line of exactly n bytes with its newline (the id padded)."""
    tail = ",%d,47.%06d,8.%06d,%d\n" % (t, t % 1000000, (7 * t) % 1000000, t % 50)
    uid = "w%d" % veh
    return (uid + "p" * (n - len(uid) - len(tail)) + tail).encode()


def test_window_edges(small_world):
    text = b"".join(_line(64, k % 7, 1000 + k) for k in range(64))                 # '\n' at byte 4095
    text += b"".join(_line(64, k % 5, 2000 + k) for k in range(63)) + _line(65, 3, 2100)
    assert text[4095:4096] == b"\n" and len(text) == 8193 and text[8192:8193] == b"\n"
    text += b"".join(_line(64, k % 3, 3000 + k) for k in range(64))                 # one straddles byte 12288
    assert len(text) == 12289 and text[12288:12289] == b"\n" and text[12287:12288] != b"\n"
    text += b"a,1,2,3,4\n" * 250 + b"b,5,6,7,8\n" * 250                             # 409 of them in one window
    text += _line(256, 1, 4000) + _line(257, 2, 4001)
    text += _line(40, 2, 4002).rstrip(b"\n")                                        # no final newline
    assert 4 * 4096 < len(text) <= 5 * 4096
    eng = engine.Engine(small_world, 0)
    bm = engine.BatchMatcher(eng)
    # the same bytes as one chunk, and cut at line ends into three (the host line is in the third)
    for chunks in ([text], [text[:4096], text[4096:8193], text[8193:]]):
        ref = engine.parse_lines_host(chunks)
        got = bm.parse_lines(chunks)
        _same_points(got, ref)
        info = bm.lines_info()
        counts = ("lines", "blank", "outside", "points", "vehicles")
        assert {k: info[k] for k in counts} == {k: ref["info"][k] for k in counts}
        assert bm.vehicle_names(chunks) == ref["names"]
        assert info["points"] == 64 + 64 + 64 + 500 + 2 + 1
        assert info["host_lines"] == 1 and info["ids_on_host"] == 0   # the 257-byte line alone
    bm.close()
    eng.close()


def test_mixed_file(small_world):
    good = lambda k: "v%d,%d,47.%05d,8.%05d,%d" % (k % 11, 5000 + k, k, 2 * k, k % 30)
    odd = [" v3 , 5001 , 47.5 ,\t8.5 , 3 ",                         # spaced
           "v4,5002,4.75e1,8.5,3",                                   # exponent
           "v5,5003,47.123456789012345,8.1234567890123456,3",        # 17 digits
           "v6,+5004,+47.5,8.5,3",                                   # '+'
           "%s,5005,47.5,8.5,3" % ("i" * 300),                       # a 300-byte id
           "v7,5006,47.,.5,3",                                       # no digits on one side of the '.'
           "   "]                                                    # blank, but not empty
    lines, n_odd = [], 0
    for k in range(1500):
        lines.append(good(k) + ("\r" if k % 9 == 0 else ""))         # CRLF lines are in the compact layout
        if k % 50 == 7:
            lines.append(odd[(k // 50) % len(odd)])
            n_odd += 1
        if k % 100 == 3:
            lines.append("")
    text = ("\n".join(lines) + "\n").encode()
    eng = engine.Engine(small_world, 0)
    bm = engine.BatchMatcher(eng)
    ref = engine.parse_lines_host([text])
    _same_points(bm.parse_lines([text]), ref)
    info = bm.lines_info()
    assert info["host_lines"] == n_odd == 30 and info["blank"] == ref["info"]["blank"] == 15 + 4
    assert info["lines"] == len(lines) and info["ids_on_host"] == 0
    assert bm.vehicle_names([text]) == ref["names"] and "i" * 300 in ref["names"]
    bm.close()
    eng.close()


def test_formatter_vector(small_world):
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "tests", "golden", "formatter_vectors.json")) as f:
        v = json.load(f)["vector"]
    fmt = engine.LineFormat.from_spec(v["spec"])
    second = v["line"].replace("06:05:40", "06:05:45")
    chunks = [(v["line"] + "\n" + second + "\n").encode()]
    eng = engine.Engine(small_world, 0)
    bm = engine.BatchMatcher(eng)
    bm.run_lines(chunks, fmt)
    lp = bm.line_points()
    assert lp["uuid"].tolist() == [0, 0] and bm.vehicle_names(chunks) == [v["id"]]
    assert lp["time"].tolist() == [v["time"], v["time"] + 5]
    assert lp["lat"].tolist() == [v["lat"]] * 2 and lp["lon"].tolist() == [v["lon"]] * 2
    assert lp["accuracy"].tolist() == [v["accuracy"]] * 2
    assert bm.lines_info()["host_lines"] == 0
    sz = bm.sizes()
    assert sz["traces"] == 1 and sz["points"] == 2
    assert bm.batch()["time"].tolist() == [v["time"], v["time"] + 5] and bm.trace_uuid().tolist() == [0]
    bm.close()
    eng.close()


def test_box_cap_and_absent_accuracy(small_world):
    text = (b"out1,100,10.0,8.5,5\n"       # outside: its id must not take index 0
            b"inA,101,47.5,8.5,1e4\n"      # accuracy 1e4 (a host line) -> cap
            b"out1,102,47.5,8.5,2.5\n"     # the same id inside: first seen here, after inA
            b"inB,103,47.5,20.0,7\n"       # outside by lon
            b"inB,104,47.25,8.25,20000\n"
            b"inA,105,48.0,9.0,0.5\n")
    fmt = engine.LineFormat(accuracy_cap=1000, bbox=(47.0, 8.0, 48.0, 9.0))
    eng = engine.Engine(small_world, 0)
    bm = engine.BatchMatcher(eng)
    got = bm.parse_lines([text], fmt)
    assert bm.vehicle_names([text]) == ["inA", "out1", "inB"]
    assert got["uuid"].tolist() == [0, 1, 2, 0] and got["time"].tolist() == [101.0, 102.0, 104.0, 105.0]
    assert got["accuracy"].tolist() == [1000.0, 3.0, 1000.0, 1.0]
    info = bm.lines_info()
    assert (info["lines"], info["outside"], info["points"], info["vehicles"], info["host_lines"]) == (6, 2, 4, 3, 1)
    _same_points(got, engine.parse_lines_host([text], fmt))
    none = engine.LineFormat(acc_col=-1)
    got = bm.parse_lines([b"a,1,2,3\nb,2,3,4,99\n"], none)
    assert got["accuracy"].tolist() == [-1.0, -1.0] and got["lat"].tolist() == [2.0, 3.0]
    assert bm.lines_info()["host_lines"] == 0
    bm.close()
    eng.close()


def test_hash_collisions_take_the_host_numbering(small_world, stream_case, monkeypatch):
    c = stream_case
    monkeypatch.setenv("RM_LINES_HASH_BITS", "4")   # 40 vehicles over 16 hash values
    eng = engine.Engine(small_world, 0)
    bm = engine.BatchMatcher(eng)
    bm.run_lines(c["chunks"], inactivity=120)
    info = bm.lines_info()
    assert info["ids_on_host"] == 1 and info["host_lines"] == 0 and info["vehicles"] == 40
    assert bm.vehicle_names(c["chunks"]) == c["names"]
    np.testing.assert_array_equal(bm.line_points()["uuid"], c["idx"])
    assert _outputs(bm) == c["want"]
    monkeypatch.delenv("RM_LINES_HASH_BITS")
    bm.run_lines(c["chunks"], inactivity=120)        # read at every call
    assert bm.lines_info()["ids_on_host"] == 0
    bm.close()
    eng.close()


BAD = {"too few fields": "v1,100,47.5,8.5", "12x": "v1,100,12x,8.5,5", "empty id": ",100,47.5,8.5,5",
       "20-digit time": "v1,12345678901234567890,47.5,8.5,5"}
BAD_T1 = {"month 13": "v1,2017-13-01 00:00:00,47.5,8.5,5", "hour 24": "v1,2017-01-01 24:00:00,47.5,8.5,5"}


def test_errors_and_empties(small_world, stream_case):
    eng = engine.Engine(small_world, 0)
    bm = engine.BatchMatcher(eng)
    for kind, bad in sorted(BAD.items()) + sorted(BAD_T1.items()):
        t1 = kind in BAD_T1
        good = "v0,2017-01-01 00:00:00,47.5,8.5,5" if t1 else "v0,100,47.5,8.5,5"
        fmt = engine.LineFormat(time_format=1 if t1 else 0)
        chunks = [(good + "\n").encode() * 4, ("\n".join([good, good, bad, good, bad]) + "\n").encode(), (bad + "\n").encode()]
        with pytest.raises(RuntimeError, match=r"^chunk 2 line 3: ") as r:
            bm.run_lines(chunks, fmt)
        with pytest.raises(RuntimeError) as h:
            engine.parse_lines_host(chunks, fmt)
        assert str(r.value) == str(h.value), kind
    with pytest.raises(RuntimeError):
        bm.lines_info()                                   # a failed call leaves nothing to read
    bm.run_lines(stream_case["chunks"], inactivity=120)   # the runner still runs a good file
    assert bm.sizes()["traces"] == 80 and bm.trace_uuid().tobytes() == stream_case["want"]["trace_uuid"]
    for chunks in ([], [b""], [b"", b"\n\n"], [b"v1,100,47.5,8.5,5"], [b"v1,100,47.5,8.5,5\n"]):
        bm.run_lines(chunks)
        assert bm.sizes()["traces"] == 0 and len(bm.trace_uuid()) == 0
        assert bm.lines_info()["points"] == (1 if chunks and chunks[-1].startswith(b"v1") else 0)
    with pytest.raises(RuntimeError, match="format"):
        bm.run_lines([b"a,1,2,3,4\n"], engine.LineFormat(uuid_col=-1))
    bm.close()
    eng.close()


def test_cli_device_ingest_writes_the_same_files(small_world, tmp_path):
    pts = _stream(small_world, n_veh=24, seed=8)
    lines = _text_lines(pts)
    tdir = tmp_path / "traces"
    tdir.mkdir()
    for f in range(3):
        (tdir / ("%03x" % f)).write_text("".join(lines[f::3]))
    conf = tmp_path / "conf.json"
    conf.write_text(json.dumps({"meili": {"default": {}}, "reporter_amd": {"graph": small_world}}))
    files = [str(p) for p in tdir.iterdir()]
    host = batch.run(files, str(conf), str(tmp_path / "host"), privacy=2, ingest="host")
    dev = batch.run(files, str(conf), str(tmp_path / "dev"), privacy=2, ingest="device")
    assert dev == host and len(host) > 0
    for name, body in host.items():
        assert (tmp_path / "dev" / name).read_text() == body == (tmp_path / "host" / name).read_text()
