"""The generic rule of separated-value trace lines on the host (rm_lines_parse_host, DESIGN.md
rule 11) against its plain-Python restatement (tests/lines_ref.py): values, vehicle numbering,
counts, the malformed kinds with their chunk and line, the calendar rule, and the reference's
formatter strings (tests/golden/formatter_vectors.json).  No GPU."""
import calendar
import json
import os
import random

import numpy as np
import pytest

import lines_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _num(rng, lo, hi):
    """A coordinate in one of the spellings the generic grammar reads."""
    v = rng.uniform(lo, hi)
    k = rng.randrange(8)
    if k == 0:
        return "%.6f" % v
    if k == 1:
        return repr(v)                      # 17 significant digits
    if k == 2:
        return "%.8e" % v                   # exponent
    if k == 3:
        return "+%.5f" % abs(v)
    if k == 4:
        return "%d." % int(v)               # no fraction digits
    if k == 5:
        return (".%04d" % rng.randrange(10000))
    if k == 6:
        return "%.3fE+00" % v
    return "%d" % int(v)


def _pad(rng, s):
    return rng.choice(["", " ", "\t", "  "]) + s + rng.choice(["", " ", "\t"])


def make_lines(seed, n, time_format=0, sep=",", extra=True):
    """n generated lines (text without the newline), some blank, in the default column order."""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        if rng.random() < 0.05:
            out.append(rng.choice(["", " ", "\t \r"]))
            continue
        uid = "veh-%d" % rng.randrange(60)
        t = rng.randrange(0, 4102444800)
        if time_format == 1:
            y, mo, d, h, mi, s = __import__("time").gmtime(t)[:6]
            tm = "%04d-%02d-%02d%s%02d:%02d:%02d" % (y, mo, d, rng.choice(" T"), h, mi, s)
        else:
            tm = rng.choice(["%d", "+%d", "%d", "0%d"]) % t if rng.random() < 0.9 else "-%d" % rng.randrange(1000)
        f = [uid, tm, _num(rng, -90, 90), _num(rng, -180, 180), _num(rng, 0, 2000)]
        if rng.random() < 0.3:
            f = [_pad(rng, x) for x in f]
        if extra and rng.random() < 0.2:
            f += ["extra", ""]
        line = sep.join(f)
        if rng.random() < 0.2:
            line = _pad(rng, line)
        out.append(line + ("\r" if rng.random() < 0.2 else ""))
    return out


def _chunks(lines):
    """Three chunks with an empty one between: the first ends in a newline, the last does not."""
    a, b = len(lines) // 3, 2 * len(lines) // 3
    join = lambda ls: "\n".join(ls).encode()
    return [join(lines[:a]) + b"\n", b"", join(lines[a:b]) + b"\n", join(lines[b:])]


def _same(got, ref):
    assert {k: got["info"][k] for k in ref["info"]} == ref["info"]
    assert got["names"] == ref["names"]
    for k in ("uuid", "time", "lon", "lat", "accuracy"):
        assert got[k].dtype == ref[k].dtype
        assert got[k].tobytes() == ref[k].tobytes(), k


@pytest.mark.parametrize("time_format", [0, 1])
def test_host_parse_equals_restatement(built_lib, time_format):
    from reporter_amd import engine
    lines = make_lines(11 + time_format, 3000, time_format)
    chunks = _chunks(lines)
    fmt = engine.LineFormat(time_format=time_format, accuracy_cap=1000, bbox=(-60.0, -150.0, 70.0, 160.0))
    ref = lines_ref.parse(chunks, fmt)
    assert ref["info"]["points"] > 1500 and ref["info"]["outside"] > 100 and ref["info"]["blank"] > 50
    _same(engine.parse_lines_host(chunks, fmt), ref)
    # another separator and column order, no accuracy column
    fmt2 = engine.LineFormat(sep=b"|", uuid_col=0, time_col=1, lat_col=3, lon_col=2, acc_col=-1, time_format=time_format)
    chunks2 = _chunks(make_lines(5, 500, time_format, sep="|"))
    ref2 = lines_ref.parse(chunks2, fmt2)
    assert (ref2["accuracy"] == -1).all() and len(ref2["accuracy"]) > 300
    _same(engine.parse_lines_host(chunks2, fmt2), ref2)


BAD = {
    "too few fields": "v1,100,1.0,2.0",
    "12x": "v1,100,12x,2.0,5",
    "empty id": " ,100,1.0,2.0,5",
    "20-digit time": "v1,12345678901234567890,1.0,2.0,5",
    "inf": "v1,100,inf,2.0,5",
    "hex": "v1,100,1.0,0x10,5",
    "underscore": "v1,100,1.0,2.0,1_0",
    "bare sign": "v1,100,-,2.0,5",
}
BAD_T1 = {
    "month 13": "v1,2017-13-01 00:00:00,1.0,2.0,5",
    "hour 24": "v1,2017-01-01 24:00:00,1.0,2.0,5",
    "day 0": "v1,2017-01-00 00:00:00,1.0,2.0,5",
    "short": "v1,2017-01-01 00:00:0,1.0,2.0,5",
}


@pytest.mark.parametrize("kind", sorted(BAD) + sorted(BAD_T1))
def test_malformed_lines_fail_with_chunk_and_line(built_lib, kind):
    from reporter_amd import engine
    t1 = kind in BAD_T1
    good = "v0,2017-01-01 00:00:00,1.0,2.0,5" if t1 else "v0,100,1.0,2.0,5"
    bad = BAD_T1[kind] if t1 else BAD[kind]
    fmt = engine.LineFormat(time_format=1 if t1 else 0)
    # the earliest bad line wins: a second bad line follows it, and another chunk of them
    chunks = [(good + "\n").encode() * 3, ("\n".join([good, "", good, bad, good, bad]) + "\n").encode(), (bad + "\n").encode()]
    with pytest.raises(lines_ref.Malformed) as r:
        lines_ref.parse(chunks, fmt)
    assert (r.value.chunk, r.value.line) == (2, 4)
    with pytest.raises(RuntimeError, match=r"^chunk 2 line 4: "):
        engine.parse_lines_host(chunks, fmt)


def test_time_rule_equals_timegm(built_lib):
    from reporter_amd import engine
    rng = random.Random(3)
    dates = [(1970, 1, 1, 0, 0, 0), (2100, 12, 31, 23, 59, 59), (2000, 2, 29, 12, 0, 0), (2016, 2, 29, 23, 59, 60),
             (2024, 2, 29, 0, 0, 0), (2100, 2, 28, 0, 0, 0), (1999, 12, 31, 23, 59, 59), (2023, 2, 31, 1, 2, 3),
             (2023, 4, 31, 0, 0, 0)]   # day 31 of a short month rolls over, as timegm's arithmetic does
    for _ in range(2000):
        y, mo = rng.randrange(1970, 2101), rng.randrange(1, 13)
        dates.append((y, mo, rng.randrange(1, calendar.monthrange(y, mo)[1] + 1), rng.randrange(24), rng.randrange(60),
                      rng.randrange(61)))
    text = "".join("v,%04d-%02d-%02d %02d:%02d:%02d,0,0,0\n" % d for d in dates).encode()
    got = engine.parse_lines_host([text], engine.LineFormat(time_format=1))["time"]
    want = [calendar.timegm((y, mo, 1, 0, 0, 0)) + (d - 1) * 86400 + h * 3600 + mi * 60 + s for y, mo, d, h, mi, s in dates]
    assert got.tolist() == [float(w) for w in want]
    inside = [k for k, d in enumerate(dates) if d[2] <= calendar.monthrange(d[0], d[1])[1]]
    assert all(got[k] == calendar.timegm(dates[k]) for k in inside) and len(inside) > 2000


def test_formatter_specs_and_vector(built_lib):
    from reporter_amd import engine
    with open(os.path.join(ROOT, "tests", "golden", "formatter_vectors.json")) as f:
        gold = json.load(f)
    for a in gold["accepted"]:
        if a["type"] == "sv":
            engine.LineFormat.from_spec(a["spec"])
        else:   # the reference reads json lines too; this reader is for separated values only
            with pytest.raises(ValueError):
                engine.LineFormat.from_spec(a["spec"])
    for spec in gold["rejected"] + [",sv,ab,0,1,2,3,4", ",sv,;,0,1,2,3,x", ",sv,;,0,1,2,3,4,HH:mm"]:
        with pytest.raises(ValueError):
            engine.LineFormat.from_spec(spec)
    v = gold["vector"]
    fmt = engine.LineFormat.from_spec(v["spec"])
    assert (fmt.sep, fmt.uuid_col, fmt.lat_col, fmt.lon_col, fmt.time_col, fmt.acc_col, fmt.time_format) == (b"|", 1, 9, 10, 0, 5, 1)
    got = engine.parse_lines_host([v["line"].encode()], fmt)
    assert got["names"] == [v["id"]] and got["uuid"].tolist() == [0]
    assert got["lat"].tolist() == [v["lat"]] and got["lon"].tolist() == [v["lon"]]
    assert got["accuracy"].tolist() == [v["accuracy"]] and got["time"].tolist() == [v["time"]]
    _same(got, lines_ref.parse([v["line"].encode()], fmt))


def test_default_format_and_limits(built_lib):
    from reporter_amd import _lib, engine
    import ctypes as C
    f = _lib.RmLineFormat()
    _lib.lib().rm_default_line_format(C.byref(f))
    assert (f.sep, f.uuid_col, f.time_col, f.lat_col, f.lon_col, f.acc_col) == (ord(","), 0, 1, 2, 3, 4)
    assert (f.time_format, f.accuracy_cap, f.use_bbox) == (0, 0, 0)
    long_id = "x" * 4096
    ok = engine.parse_lines_host([("%s,1,2,3,4" % long_id).encode()])
    assert ok["names"] == [long_id]
    with pytest.raises(RuntimeError, match="chunk 1 line 1"):
        engine.parse_lines_host([("%sy,1,2,3,4" % long_id).encode()])
    with pytest.raises(RuntimeError, match="format"):
        engine.parse_lines_host([b"a,1,2,3,4"], engine.LineFormat(time_format=2))
    empty = engine.parse_lines_host([])
    assert empty["info"]["lines"] == 0 and len(empty["uuid"]) == 0


def test_line_calls_are_exported(built_lib):
    import ctypes
    from reporter_amd import _lib
    names = ["rm_default_line_format", "rm_runner_run_lines", "rm_runner_parse_lines", "rm_runner_lines_info",
             "rm_runner_get_line_points", "rm_runner_get_vehicles", "rm_runner_lines_time", "rm_lines_parse_host"]
    h = ctypes.CDLL(built_lib)
    assert [n for n in names if not hasattr(h, n)] == []
    assert set(names) <= {n for n, _, _ in _lib.PROTOTYPES}
    header = open(os.path.join(ROOT, "include", "reporter_match.h")).read()
    assert all(n + "(" in header for n in names) and "#define RM_ABI_VERSION 1" in header
    assert ctypes.sizeof(_lib.RmLineFormat) == 72
