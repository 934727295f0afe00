"""Gzip chunks through the line reader (DESIGN.md rule 20): under BatchMatcher.set_input_coding
"gzip" and "auto", run_lines, lines_info, line_points, vehicle_names, the error messages, the
streaming push and the batch reporter give what the plain text gives, bit for bit.  Both routes
run: k_inflate + k_text_gather (RM_INFLATE_DEVICE_MIN_CHUNKS=0) and the host pool in front of the
plain upload (the default for a call of three chunks)."""
import gzip
import json

import numpy as np
import pytest

import deflate_make as dm
from reporter_amd import batch, engine
from test_gpu_lines import _outputs, _text_lines, make_stream_case
from test_gpu_stages import _stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case(small_world, tmp_path_factory):
    c = make_stream_case(small_world, tmp_path_factory.mktemp("gzlines"))
    # the first chunk as two members with padding, the second from zlib, the third (no final newline) stored
    a = c["chunks"][0]
    c["gz"] = [dm.gz(a[:len(a) // 2]) + b"\0" * 7 + dm.gz(a[len(a) // 2:], 9), gzip.compress(c["chunks"][1]), dm.gz(c["chunks"][2], 0)]
    return c


@pytest.fixture(params=["device", "host"])
def route(request, monkeypatch):
    if request.param == "device":
        monkeypatch.setenv("RM_INFLATE_DEVICE_MIN_CHUNKS", "0")
    else:
        monkeypatch.delenv("RM_INFLATE_DEVICE_MIN_CHUNKS", raising=False)
    return request.param


@pytest.fixture()
def bm(small_world):
    eng = engine.Engine(small_world, 0)
    m = engine.BatchMatcher(eng)
    yield m
    m.close()
    eng.close()


def _plain(bm, chunks):
    bm.set_input_coding("plain")
    bm.run_lines(chunks, inactivity=120)
    return _outputs(bm), bm.lines_info(), {k: v.tobytes() for k, v in bm.line_points().items()}, bm.vehicle_names(chunks)


def _check_info(bm, route, n_gz, n_members, second):
    info = bm.inflate_info()
    assert info["chunks"] == n_gz and info["members"] == n_members
    assert info["host_chunks"] == (n_gz if route == "host" else 0)
    assert info["second_pass"] == (second if route == "device" else 0)
    ms = bm.inflate_ms()
    assert set(ms) == {"inflate", "crc", "gather"} and all(v >= 0 for v in ms.values())
    assert (ms["inflate"] > 0 and ms["gather"] > 0) == (route == "device" and n_gz > 0)


@pytest.mark.parametrize("coding", ["gzip", "auto"])
def test_gzip_run_equals_plain_run(bm, case, route, coding):
    want = _plain(bm, case["chunks"])
    assert want[0] == case["want"]
    chunks = list(case["gz"])
    if coding == "auto":
        chunks[1] = case["chunks"][1]            # one chunk left plain
    bm.set_input_coding(coding)
    bm.run_lines(chunks, inactivity=120)
    assert _outputs(bm) == want[0]
    assert bm.lines_info() == want[1]
    assert {k: v.tobytes() for k, v in bm.line_points().items()} == want[2]
    assert bm.vehicle_names() == want[3] == case["names"]
    assert bm.chunk_status() == [0, 0, 0]
    _check_info(bm, route, 3 if coding == "gzip" else 2, 4 if coding == "gzip" else 3, 1)
    assert bm.inflate_info()["bytes_out"] == sum(len(c) for k, c in enumerate(case["chunks"]) if coding == "gzip" or k != 1)
    # the device text reads back, with the newline the third chunk lacked
    assert bm.text(0, 0, 40) == case["chunks"][0][:40]
    n = len(case["chunks"][2])
    assert bm.text(2, n - 10, 11) == case["chunks"][2][-10:] + b"\n"
    with pytest.raises(RuntimeError, match="span"):
        bm.text(2, n, 2)


def test_host_lines_and_bad_lines(bm, route):
    good = lambda k: "v%d,%d,47.%05d,8.%05d,%d" % (k % 11, 5000 + k, k, 2 * k, k % 30)
    odd = [" v3 , 5001 , 47.5 ,\t8.5 , 3 ", "v4,5002,4.75e1,8.5,3", "%s,5005,47.5,8.5,3" % ("i" * 300)]
    lines = []
    for k in range(900):
        lines.append(good(k))
        if k % 100 == 7:
            lines.append(odd[(k // 100) % 3])
    text = ("\n".join(lines) + "\n").encode()
    chunks = [text[:text.index(b"\n", 9000) + 1], text[text.index(b"\n", 9000) + 1:]]
    bm.set_input_coding("plain")
    want = {k: v.tobytes() for k, v in bm.parse_lines(chunks).items()}
    info, names = bm.lines_info(), bm.vehicle_names(chunks)
    assert info["host_lines"] >= 3
    bm.set_input_coding("gzip")
    got = {k: v.tobytes() for k, v in bm.parse_lines([gzip.compress(c) for c in chunks]).items()}
    assert got == want and bm.lines_info() == info and bm.vehicle_names() == names
    # a malformed line keeps the plain run's chunk and line number
    bad = [b"v0,100,47.5,8.5,5\n" * 4, b"v0,100,47.5,8.5,5\nv0,100,47.5,8.5,5\nv1,100,12x,8.5,5\nv0,100,47.5,8.5,5\n"]
    bm.set_input_coding("plain")
    with pytest.raises(RuntimeError, match=r"^chunk 2 line 3: ") as p:
        bm.parse_lines(bad)
    bm.set_input_coding("gzip")
    with pytest.raises(RuntimeError, match=r"^chunk 2 line 3: ") as g:
        bm.parse_lines([gzip.compress(c) for c in bad])
    assert str(g.value) == str(p.value)


def test_corrupt_chunk(bm, case, route):
    chunks = list(case["gz"])
    z = bytearray(chunks[1])
    z[len(z) // 2] ^= 0x10
    chunks[1] = bytes(z)
    with pytest.raises(Exception):   # (Python's gzip refuses it too)
        gzip.decompress(chunks[1])
    bm.set_input_coding("gzip")
    with pytest.raises(RuntimeError, match=r"^chunk 2: gzip: "):
        bm.run_lines(chunks, inactivity=120)
    bm.set_input_coding("plain")
    bm.run_lines([case["chunks"][0], b"", case["chunks"][2]], inactivity=120)
    want = _outputs(bm), bm.lines_info()
    bm.set_input_coding("gzip", skip_bad=True)
    bm.run_lines(chunks, inactivity=120)
    assert (_outputs(bm), bm.lines_info()) == want
    status = bm.chunk_status()
    assert status[0] == 0 and status[2] == 0 and status[1] != 0
    assert status[1] == engine.inflate_host(chunks)[1][1]


def test_push_messages(bm, case, route):
    fmt = engine.MessageFormat(kind=0, line=engine.LineFormat())
    got = []
    for coding, chunks in (("plain", case["chunks"]), ("gzip", case["gz"])):
        bm.set_input_coding(coding)
        sess = engine.VehicleSessions(bm, 64)
        vdir = engine.VehicleDirectory(64)
        out, info = sess.push_messages(chunks, fmt, vdir)
        store = sess.store()
        got.append((out, info, {k: np.asarray(v).tobytes() for k, v in store.items()}, vdir.names()))
        vdir.close()
        sess.close()
    assert got[0][0]["arrivals"] > 19000 and got[0] == got[1]


def test_chunk_status_after_a_push(bm, case, route):
    """a push is a parse of the matcher too: on a matcher that never ran lines, chunk_status() after a
    push with one bad chunk skipped has the push's three words, and the push equals that of the others"""
    fmt = engine.MessageFormat(kind=0, line=engine.LineFormat())
    bad = list(case["gz"])
    bad[1] = bad[1][:len(bad[1]) // 2]
    got = []
    for coding, chunks in (("plain", [case["chunks"][0], b"", case["chunks"][2]]), ("gzip", bad)):
        bm.set_input_coding(coding, skip_bad=True)
        sess = engine.VehicleSessions(bm, 64)
        vdir = engine.VehicleDirectory(64)
        got.append(sess.push_messages(chunks, fmt, vdir))
        assert bm.chunk_status() == ([0, 0, 0] if coding == "plain" else [0, 2, 0])
        vdir.close()
        sess.close()
    assert got[0] == got[1] and got[0][0]["arrivals"] > 12000
    bm.set_input_coding("gzip")
    sess = engine.VehicleSessions(bm, 64)
    vdir = engine.VehicleDirectory(64)
    with pytest.raises(RuntimeError, match=r"^chunk 2: gzip: "):
        sess.push_messages(bad, fmt, vdir)
    vdir.close()
    sess.close()


def test_default_coding_takes_gzip_bytes_as_text(bm, case):
    """plain is the default: a chunk of gzip bytes is text, as before"""
    z = case["gz"][1]
    want = None
    try:
        engine.parse_lines_host([z])
    except RuntimeError as e:
        want = str(e)
    assert want is not None
    with pytest.raises(RuntimeError) as r:
        bm.parse_lines([z])
    assert str(r.value) == want
    bm.set_input_coding("gzip")
    bm.set_input_coding("plain")
    with pytest.raises(RuntimeError) as r:
        bm.parse_lines([z])
    assert str(r.value) == want
    with pytest.raises(ValueError):
        bm.set_input_coding("bzip2")


def test_batch_run_over_gz_files(small_world, tmp_path, route, caplog):
    pts = _stream(small_world, n_veh=24, seed=8)
    lines = _text_lines(pts)
    plain, gz = tmp_path / "plain", tmp_path / "gz"
    plain.mkdir()
    gz.mkdir()
    for f in range(3):
        text = "".join(lines[f::3]).encode()
        (plain / ("%03x" % f)).write_bytes(text)
        (gz / ("%03x.gz" % f)).write_bytes(gzip.compress(text))
    (gz / "fff.gz").write_bytes(gzip.compress(b"v1,100,47.5,8.5,5\n")[:-6])   # a file cut short: logged and skipped
    conf = tmp_path / "conf.json"
    conf.write_text(json.dumps({"meili": {"default": {}}, "reporter_amd": {"graph": small_world}}))
    want = batch.run([str(p) for p in plain.iterdir()], str(conf), str(tmp_path / "out_plain"), privacy=2)
    with caplog.at_level("ERROR"):
        got = batch.run([str(p) for p in gz.iterdir()], str(conf), str(tmp_path / "out_gz"), privacy=2, coding="gzip")
    assert got == want and len(want) > 0
    for name, body in want.items():
        assert (tmp_path / "out_gz" / name).read_text() == body
    assert any("fff.gz was not processed: " in r.getMessage() for r in caplog.records)
    assert batch.main(["--trace-dir", str(gz), "--match-config", str(conf), "--dest-dir", str(tmp_path / "out_cli"), "--input", "auto"]) == 0
    for name, body in want.items():
        assert (tmp_path / "out_cli" / name).read_text() == body
    with pytest.raises(ValueError):
        batch.run([], str(conf), str(tmp_path / "x"), ingest="host", coding="gzip")
