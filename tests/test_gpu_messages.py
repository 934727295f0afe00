"""Stream messages read on the GPU (DESIGN.md §3 rule 14; lines.hip k_line_parse) against the host
reader (rm_messages_parse_host) and the plain-Python model (tests/messages_ref.py), for both kinds.

Inputs: conftest's small_world and the interleaved arrivals of test_gpu_sessions.py (32 vehicles x
400 points at 1 Hz, seed 11) written as text by tests/msg_text.py, cut into three chunks.  Every
tenth message (1280 of 12800) is valid but outside the compact layout, and six malformed lines are
mixed in, so the host reads 1286 lines and a tolerant call drops 6."""
import numpy as np
import pytest

import messages_ref
import msg_text
import stream_ref as sr
from reporter_amd import _lib, engine, world

pytestmark = pytest.mark.gpu

B_PARAMS = dict(report_dist_m=1200.0, report_count=20, report_time_s=150.0)


def _chunks(text):
    """Three chunks cut at line ends, an empty one between, the last without its final newline."""
    lines = text.split(b"\n")[:-1]
    a, b = len(lines) // 3, 2 * len(lines) // 3
    join = lambda ls: b"\n".join(ls)
    return [join(lines[:a]) + b"\n", b"", join(lines[a:b]) + b"\n", join(lines[b:])]


@pytest.fixture(scope="module")
def ctx(built_lib, small_world):
    tr = world.generate_traces(small_world, n_traces=32, n_points=400, rate_s=1.0, noise_m=5.0, seed=11)
    arr = sr.interleave(tr)
    eng = engine.Engine(small_world, 0)
    bm = engine.BatchMatcher(eng)
    yield {"arr": arr, "want": msg_text.expected(arr), "fmt": msg_text.formats(engine), "eng": eng, "bm": bm}
    bm.close()
    eng.close()


@pytest.mark.parametrize("kind", [0, 1])
def test_clean_text_reads_back_to_the_arrays(ctx, kind):
    """On the CPU: the comparison below is not vacuous."""
    got = engine.parse_messages_host(_chunks(msg_text.text(ctx["arr"], kind)), ctx["fmt"][kind], strict=True)
    want = ctx["want"]
    assert len(got["uuid"]) == 12800 and got["info"]["dropped"] == 0
    assert got["uuid"].tolist() == want["vehicle"].tolist()
    assert got["names"] == [msg_text.name(v) for v in range(32)]
    for k in ("time", "lon", "lat", "accuracy"):
        assert got[k].tobytes() == want[k].tobytes(), k


@pytest.mark.parametrize("kind", [0, 1])
def test_device_reader_equals_host_reader(ctx, kind):
    fmt = ctx["fmt"][kind]
    chunks = _chunks(msg_text.text(ctx["arr"], kind, bad_every=2500))
    host = engine.parse_messages_host(chunks, fmt)
    model = messages_ref.parse(chunks, fmt)
    assert host["dropped"] == model["dropped"] and len(model["dropped"]) == 6 and {d[0] for d in model["dropped"]} == {1, 3, 4}
    sess = engine.VehicleSessions(ctx["bm"], 32, **B_PARAMS)
    vdir = engine.VehicleDirectory(32)
    out, info = sess.push_messages(chunks, fmt, vdir)
    got = ctx["bm"].line_points()
    for k in ("uuid", "time", "lon", "lat", "accuracy"):
        assert got[k].dtype == host[k].dtype and got[k].tobytes() == host[k].tobytes(), k
    assert info == dict(lines=12806, blank=0, outside=0, points=12800, vehicles=32, host_lines=1286, ids_on_host=0, dropped=6)
    assert sess.dropped_messages() == model["dropped"]
    assert vdir.size == 32 and vdir.names() == host["names"]
    assert out["forwarded"] == 80
    print("messages kind", kind, info, sess.messages_ms())
    # strict: the first malformed message fails the call with the model's text, and nothing is pushed
    before = sess.store()
    with pytest.raises(messages_ref.Malformed) as want:
        messages_ref.parse(chunks, fmt, strict=True)
    with pytest.raises(_lib.RmError) as err:
        sess.push_messages(chunks, fmt, vdir, strict=True)
    assert str(err.value) == str(want.value) and str(want.value).startswith("chunk 1 line 1: ")
    after = sess.store()
    assert all(before[k].tobytes() == after[k].tobytes() for k in before)
    vdir.close()
    sess.close()


def test_bounding_box_and_blank_lines(ctx):
    """Outside, blank and kept lines are counted alike by both readers, with one stamp for the call."""
    arr = ctx["arr"]
    lat = float(np.median(arr["lat"]))
    fmt = engine.MessageFormat(0, engine.LineFormat(bbox=(lat, -180.0, 90.0, 180.0)))
    text = msg_text.text(arr, 0, 0, 3000).replace(b"\nveh/001", b"\n\n \r\nveh/001")
    host = engine.parse_messages_host([text], fmt)
    assert host["info"]["outside"] > 500 and host["info"]["blank"] > 100 and host["info"]["points"] > 500
    sess = engine.VehicleSessions(ctx["bm"], 32, **B_PARAMS)
    vdir = engine.VehicleDirectory(32)
    out, info = sess.push_messages([text], fmt, vdir, stamp_ms=123456)
    same = ("lines", "blank", "outside", "points", "vehicles", "dropped")
    assert {k: info[k] for k in same} == {k: host["info"][k] for k in same}
    assert info["host_lines"] >= host["info"]["blank"] // 2   # (the " \r" lines: whitespace is the host's)
    got = ctx["bm"].line_points()
    for k in ("uuid", "time", "lon", "lat", "accuracy"):
        assert got[k].tobytes() == host[k].tobytes(), k
    upd = sess.store()["last_update"]
    assert set(upd.tolist()) <= {0, 123456} and (upd == 123456).any()
    vdir.close()
    sess.close()
