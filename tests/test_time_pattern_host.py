"""Date patterns on the host (DESIGN.md §3 rule 18): rm_time_pattern_parse against the plain-Python
restatement (time_pattern_ref.py) over a table of patterns, random instants, fixed edges and
spoiled texts; the compiler's errors; the registry; the formatter strings; and the host line and
message readers under a pattern against lines_ref / messages_ref with the restatement plugged in."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import time_pattern_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PATTERNS = [
    "yyyy-MM-dd'T'HH:mm:ssZZ",
    "yyyy-MM-dd'T'HH:mm:ss.SSSZZ",
    "yyyyMMddHHmmss",
    "dd/MMM/yyyy HH:mm:ss",
    "M/d/yy h:mm:ss a",
    "yyyy-MM-dd HH:mm:ss.SSS",
    "d MMMM yyyy HH:mm:ss",
    "yyyyDDDHHmmss",
    "yyyy-DDD'T'HH:mm:ssZ",
    "y-D H:m:s",
    "yy-DD HH.mm.ss",
    "yyyy/MM/dd kk:mm:ss",
    "yyyy/M/d k:m:s",
    "yyyy-MM-dd KK:mm:ss a",
    "yyyy-MM-dd K:mm:ss a",
    "yyyy-MM-dd hh:mm:ssa",
    "yyMMddHHmmssSSS",
    "yyyy-MM-dd'T'HH:mm:ss.SSSSSSSSSZ",
    "yyyy-MM-dd HH:mm:ss.S",
    "MMM d, yyyy h:mm:ss a",
    "yyyy-MM-dd 'at' HH'h'mm'm'ss's'",
    "yyyy.MM.dd''HH:mm:ss",
    "'o''clock' yyyy-MM-dd HH:mm:ss",
    "dd.MM.yyyy HH:mm:ssZZ",
    "yyyyy-MM-dd HH:mm:ss",
    "yyy-MM-dd HH:mm:ss",
    "HH:mm:ss dd-MM-yyyy",
    "yyyy-MM-dd",
    "ss mm HH dd MM yyyy",
    "ZZ yyyy-MMMM-dd HH:mm",
]

EDGES = [
    ref.fields(2024, 2, 29, 12, 30, 15, 250, 60),
    ref.fields(2100, 2, 28, 23, 59, 59, 999, -300),
    ref.fields(1999, 12, 31, 23, 59, 59, 0, 0),
    ref.fields(2000, 12, 31, 23, 59, 59, 1, 0),      # day 366
    ref.fields(2017, 6, 15, 0, 0, 0, 0, 0),          # 12 AM; kk = 24
    ref.fields(2017, 6, 15, 12, 0, 0, 0, 0),         # 12 PM
    ref.fields(2017, 6, 15, 0, 59, 59, 500, 480),
    ref.fields(2017, 1, 1, 6, 5, 40, 123, 23 * 60 + 59),
    ref.fields(2017, 1, 1, 6, 5, 40, 123, -(23 * 60 + 59)),
    ref.fields(1969, 12, 31, 23, 59, 58, 500, 0),    # -1.5 s: -1
    ref.fields(1969, 12, 31, 23, 59, 59, 0, 0),
    ref.fields(1970, 1, 1, 0, 0, 0, 999, 0),
    ref.fields(2068, 12, 31, 1, 2, 3, 4, 0),         # yy = 68
    ref.fields(1969, 1, 1, 1, 2, 3, 4, 0),           # yy = 69
    ref.fields(1900, 3, 1, 0, 0, 0, 0, 0),
    ref.fields(2100, 12, 31, 23, 59, 59, 999, 0),
]


def _instants(rng, n):
    out = []
    for _ in range(n):
        y, mo = rng.randint(1900, 2100), rng.randint(1, 12)
        d = rng.randint(1, ref._month_len(y, mo))
        off = rng.choice([0, 0, 60 * rng.randint(-12, 14), rng.randint(-1439, 1439)])
        out.append(ref.fields(y, mo, d, rng.randint(0, 23), rng.randint(0, 59), rng.randint(0, 59),
                              rng.choice([0, rng.randint(0, 999)]), off))
    return out


def _texts(pattern, seed):
    """(good texts, [(mutation, text)])"""
    rng = random.Random(seed)
    inst = [ref.for_pattern(pattern, f) for f in EDGES + _instants(rng, 300)]
    good = [ref.render(pattern, f, rng if k % 2 else None) for k, f in enumerate(inst)]
    bad = [(kind, ref.mutate(pattern, f, kind, rng)) for k, f in enumerate(inst) for kind in (ref.MUTATIONS[k % 8], ref.MUTATIONS[(k + 3) % 8])]
    return good, bad


def test_table_covers_the_language():
    seen = set()
    for p in PATTERNS:
        toks = ref.tokens(p)
        for k, t in enumerate(toks):
            seen.add(t if t[0] != "lit" else "lit")
            if ref._numeric(t) and k + 1 < len(toks) and ref._numeric(toks[k + 1]):
                seen.add("adjacent")
        if "''" in p:
            seen.add("quote")
        if "'" in p.replace("''", ""):
            seen.add("quoted")
    want = {("y", 1), ("y", 2), ("y", 3), ("y", 4), ("y", 5), ("M", 1), ("M", 2), ("M", 3), ("M", 4), ("d", 1), ("d", 2),
            ("D", 1), ("D", 2), ("D", 3), ("H", 1), ("H", 2), ("k", 1), ("k", 2), ("h", 1), ("h", 2), ("K", 1), ("K", 2),
            ("a", 1), ("m", 1), ("m", 2), ("s", 1), ("s", 2), ("S", 1), ("S", 3), ("S", 9), ("Z", 1), ("Z", 2),
            "lit", "adjacent", "quote", "quoted"}
    assert len(PATTERNS) >= 24 and want <= seen, want - seen


@pytest.mark.parametrize("k", range(len(PATTERNS)))
def test_parse_equals_restatement(built_lib, k):
    from reporter_amd import engine
    pattern = PATTERNS[k]
    good, bad = _texts(pattern, 1000 + k)
    # the reference alone: the unspoiled texts are well formed and say what was written; every
    # mutation class occurs; at least a third of the spoiled texts are malformed
    want_good = [ref.parse(pattern, t) for t in good]
    assert all(v is not None for v in want_good), [t for t, v in zip(good, want_good) if v is None][:3]
    want_bad = [ref.parse(pattern, t) for _, t in bad]
    assert {kind for kind, _ in bad} == set(ref.MUTATIONS)
    n_mal = sum(v is None for v in want_bad)
    assert 3 * n_mal >= len(bad), (n_mal, len(bad))
    assert len(set(want_good)) > 250
    # the library
    for t, w in zip(good + [t for _, t in bad], want_good + want_bad):
        got = engine.parse_time(pattern, t)
        assert got == (None if w is None else float(w)), (pattern, t, got, w)
        assert got is None or got == int(got)


def test_reference_values():
    """The restatement against instants worked out by hand."""
    p = ref.parse
    assert p("yyyy-MM-dd'T'HH:mm:ssZZ", "2017-01-01T06:05:40Z") == 1483250740
    assert p("yyyy-MM-dd'T'HH:mm:ss.SSSZZ", "2017-01-01T06:05:40.123+08:00") == 1483250740 - 8 * 3600
    assert p("yyyyMMddHHmmss", "20170101060540") == 1483250740
    assert p("dd/MMM/yyyy HH:mm:ss", "01/Jan/2017 06:05:40") == 1483250740
    assert p("M/d/yy h:mm:ss a", "1/1/17 6:05:40 AM") == 1483250740
    assert p("M/d/yy h:mm:ss a", "1/1/17 12:05:40 am") == 1483250740 - 6 * 3600
    assert p("M/d/yy h:mm:ss a", "1/1/17 12:05:40 PM") == 1483250740 + 6 * 3600
    assert p("yyyy-MM-dd kk:mm", "2017-01-01 24:00") == 1483228800
    assert p("yyyy-MM-dd KK:mm a", "2017-01-01 11:00 PM") == 1483228800 + 23 * 3600
    assert p("yyyy-MM-dd HH:mm:ss.SSS", "1969-12-31 23:59:58.500") == -1
    assert p("yyyy-MM-dd HH:mm:ss.SSS", "1969-12-31 23:59:58.000") == -2
    assert p("yyyy-MM-dd HH:mm:ss.SSSSSSSSS", "1969-12-31 23:59:58.000999999") == -2
    assert p("yyyy-DDD", "2016-366") == 1483142400 and p("yyyy-DDD", "2017-366") is None
    assert p("yy-MM-dd", "68-01-01") == 3092601600 and p("yy-MM-dd", "69-01-01") == -31536000
    assert p("yyyy-MM-dd", "2023-02-29") is None and p("yyyy-MM-dd", "2024-02-29") == 1709164800
    assert p("yyyy-MM-dd", "2100-02-29") is None
    assert p("yyyy-MM-dd HH:mm:ss", "2017-01-01 06:05:60") is None
    assert p("y-M-d", "0-3-1") == -62162035200 and p("y-M-d", "12345-1-1") is None


COMPILE_ERRORS = [
    ("yyyy-MM-dd yyyy", "field 'y' is given twice"),
    ("yyyy-MM-dd MMM", "field 'M' is given twice"),
    ("yyyy-MM-dd HH:mm:ss ss", "field 's' is given twice"),
    ("yyyy-MM-dd hh:mm", "'h' and 'K' need 'a'"),
    ("yyyy-MM-dd KK:mm", "'h' and 'K' need 'a'"),
    ("yyyy-MM-dd HH:mm a", "'a' needs 'h' or 'K'"),
    ("yyyy-MM-dd HH kk", "two hour fields"),
    ("yyyy-MM-dd hh HH a", "two hour fields"),
    ("yyyy-DDD-MM", "'D' cannot stand with 'M' or 'd'"),
    ("yyyy-DDD dd", "'D' cannot stand with 'M' or 'd'"),
    ("MM-dd HH:mm:ss", "the pattern has no year"),
    ("HH:mm", "the pattern has no year"),
    ("", "the pattern has no year"),
    ("yyyy-MM HH:mm", "the pattern needs 'D', or both 'M' and 'd'"),
    ("yyyy dd", "the pattern needs 'D', or both 'M' and 'd'"),
    ("yyyy-MM-dd SSSHH", "'S' is directly followed by a numeric field"),
    ("yyyy-MM-dd'T'HH:mm:ss.SSSZZ" + "'" + "x" * 40 + "'", "the pattern is longer than 63 bytes"),
    ("yyyy-MM-dd'" + "x" * 30 + "'", "the pattern has more than 32 steps"),
    ("yyyy-MM-dd HH:mm:ssZZZ", "'ZZZ' (a zone id) is not read"),
    ("yyyy-MM-dd 'open", "a quote is not closed"),
    ("yyyy-MM-ddd", "field 'd' takes at most 2 letters"),
    ("yyyy-MM-dd \"HH\"", "a literal cannot be a double quote, a backslash or a control byte"),
    ("yyyy-MM-dd\tHH", "a literal cannot be a double quote, a backslash or a control byte"),
    (" yyyy-MM-dd", "the pattern begins with a space"),
    ("yyyy-MM-dd ", "the pattern ends with a space"),
    ("yyyy-MM-dd Q", "unknown pattern letter 'Q'"),
] + [("yyyy-MM-dd " + c, "field '%s' is not read" % c) for c in "zEewxYCG"]


@pytest.mark.parametrize("pattern,message", COMPILE_ERRORS)
def test_compile_errors(built_lib, pattern, message):
    from reporter_amd import engine
    with pytest.raises(ValueError) as e:
        engine.time_pattern_id(pattern)
    assert message in str(e.value)
    with pytest.raises(ValueError) as e:
        engine.LineFormat(time_pattern=pattern)
    assert message in str(e.value)


def test_ids(built_lib):
    import ctypes as C
    from reporter_amd import _lib, engine
    a = engine.time_pattern_id("yyyy-MM-dd'T'HH:mm:ssZZ")
    b = engine.time_pattern_id("yyyyMMddHHmmss")
    assert a >= 16 and b >= 16 and a != b
    assert engine.time_pattern_id("yyyy-MM-dd'T'HH:mm:ssZZ") == a and engine.time_pattern_id(b"yyyyMMddHHmmss") == b
    out = C.create_string_buffer(64)
    assert _lib.lib().rm_time_pattern_text(a, out, 64) == 0 and out.value == b"yyyy-MM-dd'T'HH:mm:ssZZ"
    assert _lib.lib().rm_time_pattern_text(15, out, 64) == 1 and _lib.lib().rm_time_pattern_text(5000, out, 64) == 1
    v = C.c_double(0)
    assert _lib.lib().rm_time_pattern_parse(5000, b"x", 1, C.byref(v)) == 2
    f = engine.LineFormat(time_pattern="yyyyMMddHHmmss")
    assert f.time_pattern == "yyyyMMddHHmmss" and f.time_format == 0 and f._c().time_format == b
    with pytest.raises(ValueError):
        engine.LineFormat(time_format=1, time_pattern="yyyyMMddHHmmss")


def test_the_241st_pattern_fails(built_lib):
    """The registry holds 240 patterns for the life of a process: filled in a process of its own."""
    code = """
import sys
sys.path.insert(0, %r)
from reporter_amd import engine
ids = [engine.time_pattern_id("yyyy-MM-dd'%%03d'" %% k) for k in range(240)]
assert ids == list(range(16, 256)), ids
try:
    engine.time_pattern_id("yyyy-MM-dd'240'")
    print("registered")
except ValueError as e:
    print("refused:", e)
assert engine.time_pattern_id("yyyy-MM-dd'007'") == 16 + 7
assert engine.parse_time("yyyy-MM-dd'239'", "1970-01-02239") == 86400.0
try:
    engine.time_pattern_id("yyyy-MM-dd HH")
    print("registered")
except ValueError as e:
    print("refused again:", e)
try:
    engine.time_pattern_id("yyyy-MM")
except ValueError as e:
    print("compile error first:", e)
""" % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "refused: " in r.stdout and "at most 240 time patterns" in r.stdout and "refused again" in r.stdout
    assert "registered" not in r.stdout and "compile error first" in r.stdout and "needs 'D'" in r.stdout


def test_unknown_time_formats_fail(built_lib):
    from reporter_amd import _lib, engine
    for tf in (2, 15, 99, 255, -1):
        with pytest.raises(_lib.RmError, match="time_format"):
            engine.parse_lines_host([b"a,1,2,3,4"], engine.LineFormat(time_format=tf))
        for kind in (0, 1):
            with pytest.raises(_lib.RmError, match="format"):
                engine.parse_messages_host([b"{}"], engine.MessageFormat(kind, engine.LineFormat(time_format=tf)))


def test_separator_in_the_pattern(built_lib):
    from reporter_amd import _lib, engine
    f = engine.LineFormat(sep=b"-", time_pattern="yyyy-MM-dd")
    with pytest.raises(_lib.RmError, match="separator"):
        engine.parse_lines_host([b"a-1-2-3-4"], f)
    with pytest.raises(_lib.RmError, match="separator"):
        engine.parse_messages_host([b"a-1-2-3-4"], engine.MessageFormat(0, f))
    # JSON has no separator
    got = engine.parse_messages_host([b'{"id":"a","latitude":1,"longitude":2,"timestamp":"1970-01-02","accuracy":3}'],
                                     engine.MessageFormat(1, f), strict=True)
    assert list(got["time"]) == [86400.0]


def test_from_spec(built_lib):
    from reporter_amd import engine
    sv = engine.LineFormat.from_spec(",sv,\\|,1,9,10,0,5,yyyy-MM-dd'T'HH:mm:ssZZ")
    assert (sv.sep, sv.uuid_col, sv.lat_col, sv.lon_col, sv.time_col, sv.acc_col) == (b"|", 1, 9, 10, 0, 5)
    assert sv.time_format == 0 and sv.time_pattern == "yyyy-MM-dd'T'HH:mm:ssZZ"
    assert sv._c().time_format == engine.time_pattern_id("yyyy-MM-dd'T'HH:mm:ssZZ") >= 16
    m = engine.MessageFormat.from_spec(",sv,\\|,1,9,10,0,5,yyyy-MM-dd'T'HH:mm:ssZZ")
    assert m.kind == 0 and m.line.time_pattern == sv.time_pattern
    j = engine.MessageFormat.from_spec("@json@id@la@lo@t@a@yyyyMMddHHmmss")
    assert j.kind == 1 and j.keys == (b"id", b"la", b"lo", b"t", b"a") and j.line.time_pattern == "yyyyMMddHHmmss"
    assert j._c().line.time_format == engine.time_pattern_id("yyyyMMddHHmmss")
    # what was read before is read as before
    old = engine.LineFormat.from_spec(",sv,\\|,1,9,10,0,5,yyyy-MM-dd HH:mm:ss")
    assert old.time_format == 1 and old.time_pattern is None and old._c().time_format == 1
    assert engine.MessageFormat.from_spec("@json@id@la@lo@t@a@yyyy-MM-dd HH:mm:ss").line.time_format == 1
    assert engine.LineFormat.from_spec(",sv,\\|,1,9,10,0,5").time_format == 0
    for spec in (",sv,\\|,1,9,10,0,5,HH:mm", "@json@id@la@lo@t@a@HH:mm"):
        with pytest.raises(ValueError):
            engine.MessageFormat.from_spec(spec)
    with pytest.raises(ValueError):
        engine.LineFormat.from_spec(",sv,\\|,1,9,10,0,5,HH:mm")


# ---------------------------------------------------------------- lines and messages under a pattern
LINE_PATTERNS = ["yyyy-MM-dd'T'HH:mm:ss.SSSZZ", "yyyyMMddHHmmss", "dd/MMM/yyyy HH:mm:ss", "M/d/yy h:mm:ss a"]


def _rows(pattern, seed, n, bad_every):
    rng = random.Random(seed)
    rows = []
    for k, f in enumerate(_instants(rng, n)):
        f = ref.for_pattern(pattern, f)
        if bad_every and k % bad_every == bad_every - 1:
            t = ref.mutate(pattern, f, ref.MUTATIONS[(k // bad_every) % 8], rng)
        else:
            t = ref.render(pattern, f, rng)
        rows.append(("veh-%d" % rng.randrange(40), t, "%.6f" % rng.uniform(-70, 80), "%.6f" % rng.uniform(-170, 170),
                     "%.1f" % rng.uniform(0, 1500)))
    return rows


def _sv_chunks(rows, rng):
    lines = []
    for k, (uid, t, la, lo, ac) in enumerate(rows):
        if k % 7 == 3:
            t = " " + t + "\t"   # whitespace round a field is stripped
        lines.append("|".join((uid, t, la, lo, ac)) + ("\r" if k % 5 == 0 else ""))
        if k % 50 == 10:
            lines.append("")
    text = ("\n".join(lines) + "\n").encode()
    cut = text.index(b"\n", len(text) // 2) + 1
    return [text[:cut], text[cut:]]


def _json_chunks(rows, rng):
    lines = []
    for k, (uid, t, la, lo, ac) in enumerate(rows):
        tv = '"%s"' % t
        if k % 11 == 5:
            tv = '"\\u00%02x%s"' % (ord(t[0]), t[1:])   # the first byte as an escape: the same string
        if k % 37 == 9:
            tv = "1483250740"   # a number node is malformed under a pattern
        if k % 41 == 7:
            tv = '" %s"' % t    # no stripping inside a string
        sp = " " if k % 6 == 0 else ""
        lines.append('{"id":"%s",%s"t":%s,"la":%s,"lo":%s,"a":%s}' % (uid, sp, tv, la, lo, ac))
    text = ("\n".join(lines) + "\n").encode()
    cut = text.index(b"\n", len(text) // 2) + 1
    return [text[:cut], text[cut:]]


def _same(got, want):
    for key in ("uuid", "time", "lon", "lat", "accuracy"):
        assert np.array_equal(got[key], want[key]), key
    assert got["names"] == want["names"]
    for key, v in want["info"].items():
        assert got["info"][key] == v, key


@pytest.mark.parametrize("pattern", LINE_PATTERNS)
def test_host_lines_equal_restatement(built_lib, pattern):
    import lines_ref
    from reporter_amd import _lib, engine
    fmt = engine.LineFormat(sep=b"|", time_pattern=pattern, accuracy_cap=1000, bbox=(-60.0, -150.0, 70.0, 160.0))
    rng = random.Random(5)
    clean = _sv_chunks(_rows(pattern, 77, 1500, 0), rng)
    _same(engine.parse_lines_host(clean, fmt), ref.lines(clean, fmt))
    dirty = _sv_chunks(_rows(pattern, 78, 600, 9), rng)
    with pytest.raises(lines_ref.Malformed) as want:
        ref.lines(dirty, fmt)
    with pytest.raises(_lib.RmError) as got:
        engine.parse_lines_host(dirty, fmt)
    assert str(got.value) == "chunk %d line %d: malformed time (%s)" % (want.value.chunk, want.value.line, pattern)


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("pattern", LINE_PATTERNS)
def test_host_messages_equal_restatement(built_lib, pattern, kind):
    from reporter_amd import engine
    line = engine.LineFormat(sep=b"|", time_pattern=pattern, accuracy_cap=1000, bbox=(-60.0, -150.0, 70.0, 160.0))
    mf = engine.MessageFormat(kind, line, ("id", "la", "lo", "t", "a"))
    rng = random.Random(6)
    chunks = (_json_chunks if kind else _sv_chunks)(_rows(pattern, 79 + kind, 1500, 6), rng)
    got = engine.parse_messages_host(chunks, mf)
    want = ref.messages(chunks, mf)
    _same(got, want)
    assert got["dropped"] == want["dropped"] and got["info"]["dropped"] > 100
    assert all(why == "malformed time (%s)" % pattern for _, _, why in got["dropped"])
