"""The generic rule of stream messages on the host (rm_messages_parse_host, DESIGN.md §3 rule 14)
against its plain-Python restatement (tests/messages_ref.py): both kinds, values, vehicle numbering,
counts, the dropped messages of a tolerant call with their reasons in order, the text a strict call
fails with, and the reference's formatter strings (tests/golden/formatter_vectors.json).  No GPU."""
import json
import os
import random
import time as _time

import numpy as np
import pytest

import messages_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _num(rng, lo, hi, compact=False):
    v = rng.uniform(lo, hi)
    k = rng.randrange(4 if compact else 8)
    if k == 0:
        return "%.6f" % v
    if k == 1:
        return "%d" % int(v)
    if k == 2:
        return "%.1f" % v
    if k == 3:
        return "%.9f" % v
    if k == 4:
        return repr(v)                      # 17 significant digits
    if k == 5:
        return "%.8e" % v                   # exponent
    if k == 6:
        return '"%s%.5f"' % (rng.choice(["", " ", "+"]), abs(v))   # a number in a string
    return "%.3fE+00" % v


BAD_JSON = [
    '{"id":"v1","timestamp":100,"latitude":1.0,"longitude":2.0',            # cut short
    '["id","v1"]',                                                          # not an object
    '{"id":"v1","timestamp":100,"latitude":1.0,"accuracy":5}',              # no longitude
    '{"id":"v1","timestamp":100,"latitude":"12x","longitude":2.0,"accuracy":5}',
    '{"id":"v1","timestamp":100,"latitude":1.0,"longitude":true,"accuracy":5}',
    '{"id":"","timestamp":100,"latitude":1.0,"longitude":2.0,"accuracy":5}',
    '{"id":"a\\u0041","timestamp":100,"latitude":1.0,"longitude":2.0,"accuracy":5}',
    '{"id":1.5,"timestamp":100,"latitude":1.0,"longitude":2.0,"accuracy":5}',
    '{"id":"v1","timestamp":"soon","latitude":1.0,"longitude":2.0,"accuracy":5}',
    '{"id":"v1","timestamp":null,"latitude":1.0,"longitude":2.0,"accuracy":5}',
    '{"id":"v1","timestamp":100,"latitude":1.0,"longitude":2.0,"accuracy":[5]}',
    'id=v1 latitude=1.0',
    # numbers that are not JSON's: a leading zero, a bare dot, also inside an unused nested member
    '{"id":"v1","timestamp":100,"latitude":01,"longitude":2.0,"accuracy":5}',
    '{"id":"v1","timestamp":100,"latitude":1.,"longitude":2.0,"accuracy":5}',
    '{"id":"v1","timestamp":007,"latitude":1.0,"longitude":2.0,"accuracy":5}',
    '{"id":"v1","timestamp":100,"latitude":1.0,"longitude":2.0,"accuracy":5,"extra":[{"n":-01}]}',
    '{"id":"v1","timestamp":100,"latitude":1.0,"longitude":2.0,"accuracy":1.e2}',
]
BAD_JSON_T1 = [
    '{"id":"v1","timestamp":"2017-13-01 00:00:00","latitude":1.0,"longitude":2.0,"accuracy":5}',
    '{"id":"v1","timestamp":1483250740,"latitude":1.0,"longitude":2.0,"accuracy":5}',
    '{"id":"v1","timestamp":"2017-01-01 00:00:0","latitude":1.0,"longitude":2.0,"accuracy":5}',
]
BAD_SV = ["v1,100,1.0,2.0", "v1,100,12x,2.0,5", " ,100,1.0,2.0,5", "v1,12345678901234567890,1.0,2.0,5", "v1,100,1.0,0x10,5",
          "v1,100,1.0,2.0,1_0"]
BAD_SV_T1 = ["v1,2017-13-01 00:00:00,1.0,2.0,5", "v1,2017-01-01 00:00:0,1.0,2.0,5"]


def _time_text(rng, time_format, quoted):
    t = rng.randrange(0, 4102444800)
    if time_format == 1:
        y, mo, d, h, mi, s = _time.gmtime(t)[:6]
        tm = "%04d-%02d-%02d%s%02d:%02d:%02d" % (y, mo, d, rng.choice(" T"), h, mi, s)
        return '"%s"' % tm if quoted else tm
    return "%d" % t if rng.random() < 0.9 else "-%d" % rng.randrange(1000)


def make_json(seed, n, time_format=0, bad_every=0):
    """n generated JSON messages: compact and loose spellings, keys in every order, extra members,
    blanks, and (bad_every > 0) a malformed one at every bad_every-th place."""
    rng = random.Random(seed)
    bad = BAD_JSON + (BAD_JSON_T1 if time_format == 1 else [])
    out = []
    for k in range(n):
        if bad_every and k % bad_every == bad_every - 1:
            out.append(bad[(k // bad_every) % len(bad)])
            continue
        if rng.random() < 0.05:
            out.append(rng.choice(["", " ", "\t \r"]))
            continue
        loose = rng.random() < 0.4
        uid = '"veh-%d"' % rng.randrange(60) if rng.random() < 0.9 else "%d" % rng.randrange(5)
        tm = _time_text(rng, time_format, True)
        if loose and time_format == 0:
            tm = rng.choice([tm, '"%s"' % tm, '" +%s "' % tm.lstrip("-"), tm + ".75", tm + "e0"])
        mem = [('"id"', uid), ('"timestamp"', tm), ('"latitude"', _num(rng, -90, 90, not loose)),
               ('"longitude"', _num(rng, -180, 180, not loose)), ('"accuracy"', _num(rng, 0, 2000, not loose))]
        for _ in range(rng.randrange(3)):
            mem.append(rng.choice([('"speed"', "12.5"), ('"ok"', "true"), ('"note"', '"a, {b}"'), ('"gone"', "null")]))
        if loose and rng.random() < 0.5:
            mem.append(('"nest"', '{"id":[1,{"latitude":"}"}],"x":null}'))
        rng.shuffle(mem)
        if loose and rng.random() < 0.3:
            mem.insert(0, ('"latitude"', '"the last one wins"'))
        colon, comma = (rng.choice([":", " : ", ": "]), rng.choice([",", " , ", ", "])) if loose else (":", ",")
        line = "{" + comma.join(k_ + colon + v for k_, v in mem) + "}"
        if loose and rng.random() < 0.3:
            line = rng.choice([" ", "\t"]) + line + " "
        out.append(line + ("\r" if rng.random() < 0.2 else ""))
    return out


def make_sv(seed, n, time_format=0, bad_every=0):
    rng = random.Random(seed)
    bad = BAD_SV + (BAD_SV_T1 if time_format == 1 else [])
    out = []
    for k in range(n):
        if bad_every and k % bad_every == bad_every - 1:
            out.append(bad[(k // bad_every) % len(bad)])
            continue
        if rng.random() < 0.05:
            out.append(rng.choice(["", " "]))
            continue
        f = ["veh-%d" % rng.randrange(60), _time_text(rng, time_format, False),
             _num(rng, -90, 90, True), _num(rng, -180, 180, True), _num(rng, 0, 2000, True)]
        if rng.random() < 0.3:
            f = [" " + x + "\t" for x in f]
        out.append(",".join(f) + ("\r" if rng.random() < 0.2 else ""))
    return out


def chunks_of(lines):
    """Three chunks with an empty one between: the first ends in a newline, the last does not."""
    a, b = len(lines) // 3, 2 * len(lines) // 3
    join = lambda ls: "\n".join(ls).encode()
    return [join(lines[:a]) + b"\n", b"", join(lines[a:b]) + b"\n", join(lines[b:])]


def same(got, ref):
    assert {k: got["info"][k] for k in ref["info"]} == ref["info"]   # (the model has no host lines to count)
    assert got["names"] == ref["names"]
    assert got["dropped"] == ref["dropped"]
    for k in ("uuid", "time", "lon", "lat", "accuracy"):
        assert got[k].dtype == ref[k].dtype
        assert got[k].tobytes() == ref[k].tobytes(), k


def _format(engine, kind, time_format):
    line = engine.LineFormat(time_format=time_format, accuracy_cap=1000, bbox=(-60.0, -150.0, 70.0, 160.0))
    return engine.MessageFormat(kind, line)


@pytest.mark.parametrize("time_format", [0, 1])
@pytest.mark.parametrize("kind", [0, 1])
def test_host_parse_equals_restatement(built_lib, kind, time_format):
    from reporter_amd import engine
    make = make_json if kind == 1 else make_sv
    fmt = _format(engine, kind, time_format)
    clean = chunks_of(make(21 + time_format, 3000, time_format))
    ref = messages_ref.parse(clean, fmt)
    assert ref["info"]["points"] > 1500 and ref["info"]["outside"] > 100 and ref["info"]["blank"] > 50
    assert ref["info"]["dropped"] == 0 and ref["info"]["vehicles"] >= 60
    same(engine.parse_messages_host(clean, fmt), ref)
    same(engine.parse_messages_host(clean, fmt, strict=True), ref)
    # tolerant: the malformed messages are dropped and listed, with their reasons, in input order
    dirty = chunks_of(make(31 + time_format, 3000, time_format, bad_every=23))
    ref = messages_ref.parse(dirty, fmt)
    assert ref["info"]["dropped"] == 3000 // 23 and len(ref["dropped"]) == 64 and len({d[2] for d in ref["dropped"]}) >= 5
    same(engine.parse_messages_host(dirty, fmt), ref)
    # strict: the first of them fails the call, with the same text
    with pytest.raises(messages_ref.Malformed) as want:
        messages_ref.parse(dirty, fmt, strict=True)
    with pytest.raises(RuntimeError) as got:
        engine.parse_messages_host(dirty, fmt, strict=True)
    assert str(got.value) == str(want.value) and str(want.value).startswith("chunk 1 line 23: ")


def test_every_malformed_kind_has_the_models_reason(built_lib):
    from reporter_amd import engine
    for t1, bad, good in ((0, BAD_JSON, '{"id":"v0","timestamp":100,"latitude":1.0,"longitude":2.0,"accuracy":5}'),
                          (1, BAD_JSON_T1, '{"id":"v0","timestamp":"2017-01-01 00:00:00","latitude":1.0,"longitude":2.0,"accuracy":5}')):
        fmt = engine.MessageFormat(1, engine.LineFormat(time_format=t1))
        text = ["\n".join([good] + bad + [good]).encode()]
        ref = messages_ref.parse(text, fmt)
        assert ref["info"]["dropped"] == len(bad) and ref["info"]["points"] == 2
        same(engine.parse_messages_host(text, fmt), ref)
    # no accuracy key: the member is not needed and the value is -1
    fmt = engine.MessageFormat(1, keys=("id", "latitude", "longitude", "timestamp", ""))
    got = engine.parse_messages_host([b'{"id":7,"timestamp":5.9,"latitude":"1.5","longitude":-2}'], fmt)
    assert got["names"] == ["7"] and got["time"].tolist() == [5.0] and got["accuracy"].tolist() == [-1.0]
    same(got, messages_ref.parse([b'{"id":7,"timestamp":5.9,"latitude":"1.5","longitude":-2}'], fmt))


def test_minus_zero(built_lib):
    """`-0` as a time is +0.0 whatever its spelling (a long has no sign of zero); as a coordinate a
    number node keeps its sign.  Digits in strings are no number tokens."""
    from reporter_amd import engine
    fmt = engine.MessageFormat(1)
    line = '{"id":"007","timestamp":%s,"latitude":%s,"longitude":-0.0,"accuracy":0,"note":"01 and 1. and -"}'
    text = ["\n".join(line % (t, la) for t in ("-0", "0", "-0.0", "-0.4", '"-0"', "-0e0") for la in ("-0", "0", '"-0"')).encode()]
    ref = messages_ref.parse(text, fmt)
    got = engine.parse_messages_host(text, fmt, strict=True)
    same(got, ref)
    assert ref["info"]["points"] == 18 and ref["names"] == ["007"]
    assert got["time"].tobytes() == np.zeros(18).tobytes()                      # every bit clear
    assert np.signbit(got["lat"]).tolist() == [True, False, True] * 6 and np.signbit(got["lon"]).all()


def test_formatter_specs_and_vector(built_lib):
    from reporter_amd import engine
    with open(os.path.join(ROOT, "tests", "golden", "formatter_vectors.json")) as f:
        gold = json.load(f)
    sv, j0, j1 = (engine.MessageFormat.from_spec(a["spec"]) for a in gold["accepted"])
    assert [a["type"] for a in gold["accepted"]] == ["sv", "json", "json"]
    assert sv.kind == 0 and (sv.line.sep, sv.line.uuid_col, sv.line.lat_col, sv.line.lon_col, sv.line.time_col, sv.line.acc_col,
                             sv.line.time_format) == (b"|", 1, 9, 10, 0, 5, 1)
    assert j0.kind == 1 and j0.keys == (b"id", b"latitude", b"longitude", b"timestamp", b"accuracy") and j0.line.time_format == 0
    assert j1.kind == 1 and j1.keys == (b"id", b"la", b"lo", b"t", b"a") and j1.line.time_format == 1
    for spec in gold["rejected"] + ["@json@id@lat@lon@t@a@HH:mm", "@json@id@id@lon@t@a", "@json@" + "k" * 32 + "@la@lo@t@a",
                                    '@json@i"d@la@lo@t@a', "@json@@la@lo@t@a"]:
        with pytest.raises(ValueError):
            engine.MessageFormat.from_spec(spec)
    v = gold["vector"]
    got = engine.parse_messages_host([v["line"].encode()], engine.MessageFormat.from_spec(v["spec"]))
    assert got["names"] == [v["id"]] and got["uuid"].tolist() == [0]
    assert got["lat"].tolist() == [v["lat"]] and got["lon"].tolist() == [v["lon"]]
    assert got["accuracy"].tolist() == [v["accuracy"]] and got["time"].tolist() == [v["time"]]
    # the same point as a JSON message under the third accepted spec
    line = b'{"t":"2017-01-01 06:05:40","i":"w00t","a":6.5,"la":0.0,"lo":0.0}'
    got = engine.parse_messages_host([line], engine.MessageFormat.from_spec("@json@i@la@lo@t@a@yyyy-MM-dd HH:mm:ss"))
    assert got["names"] == [v["id"]] and got["time"].tolist() == [v["time"]] and got["accuracy"].tolist() == [v["accuracy"]]


def test_message_calls_are_exported(built_lib):
    import ctypes
    from reporter_amd import _lib, engine
    names = ["rm_default_message_format", "rm_directory_create", "rm_directory_destroy", "rm_directory_size",
             "rm_directory_names", "rm_session_push_messages", "rm_session_dropped_messages", "rm_messages_parse_host",
             "rm_session_messages_time", "rm_session_messages_span"]
    h = ctypes.CDLL(built_lib)
    assert [n for n in names if not hasattr(h, n)] == []
    assert set(names) <= {n for n, _, _ in _lib.PROTOTYPES}
    header = open(os.path.join(ROOT, "include", "reporter_match.h")).read()
    assert all(n + "(" in header for n in names) and "#define RM_ABI_VERSION 1" in header
    assert ctypes.sizeof(_lib.RmLineFormat) == 72 and ctypes.sizeof(_lib.RmMessageFormat) == 240
    assert ctypes.sizeof(_lib.RmMessagesDesc) == 280
    f = _lib.RmMessageFormat()
    _lib.lib().rm_default_message_format(ctypes.byref(f))
    assert f.kind == 0 and [f.key[i].value for i in range(5)] == [b"id", b"latitude", b"longitude", b"timestamp", b"accuracy"]
    with pytest.raises(RuntimeError, match="format"):
        engine.parse_messages_host([b"{}"], engine.MessageFormat(1, engine.LineFormat(time_format=2)))
