"""Interleaved arrivals (stream_ref.interleave) written as raw stream messages for the GPU tests of
DESIGN.md §3 rule 14: separated values with epoch seconds (kind 0) and JSON with calendar times
(kind 1).  float32 coordinates are written in their shortest round-trip spelling, so the text reads
back to the arrays bit for bit (test_gpu_messages.py asserts it on the CPU).  Every tenth message is
in a valid form the compact reader hands to the host: spaces, an exponent, and for JSON shuffled keys
with a nested extra member."""
import time as _time

import numpy as np

KEYS = ("uuid", "la", "lo", "when", "acc")
BAD = {0: ["veh/000,12,1.0", "veh/001,12,north,2.0,5", "veh/002,tomorrow,1.0,2.0,5"],
       1: ['{"uuid":"veh/000","la":1.0,"lo":2.0,"when":"2017-01-01 00:00:00"',
           '{"uuid":"veh/001","la":"north","lo":2.0,"when":"2017-01-01 00:00:00","acc":5}',
           '{"uuid":"veh/002","la":1.0,"lo":2.0,"acc":5}']}


def name(v):
    return "veh/%03d%s" % (v, "-bus" * (v % 3))


def formats(engine):
    return {0: engine.MessageFormat(0, engine.LineFormat()),
            1: engine.MessageFormat(1, engine.LineFormat(time_format=1), KEYS)}


def expected(arr):
    """The arrays the messages read back to: the arrivals with the accuracy's ceiling (Formatter.java:106)."""
    out = dict(arr)
    out["accuracy"] = np.ceil(arr["accuracy"].astype(np.float64)).astype(np.float32)
    return out


def _civil(t):
    return "%04d-%02d-%02d %02d:%02d:%02d" % _time.gmtime(int(t))[:6]


def _with_exponent(s):
    """A spelling with an exponent: its own if it has one (near 0 degrees the shortest spelling of
    a float32 is already 4.2e-05), else "e0" appended."""
    return s if "e" in s else s + "e0"


def message(arr, j, kind, odd):
    v, t = int(arr["vehicle"][j]), arr["time"][j]
    assert t == int(t)
    lon, lat =str(np.float32(arr["lon"][j])), str(np.float32(arr["lat"][j]))
    acc = str(np.float32(arr["accuracy"][j]))   # (read back as its ceiling: expected())
    if kind == 0:
        if odd:
            return " %s , %d,%s,\t%s,%s \r" % (name(v), int(t), _with_exponent(lat), lon, acc)
        return "%s,%d,%s,%s,%s" % (name(v), int(t), lat, lon, acc)
    if odd:
        return ' {"nest":{"uuid":["x",{"la":"}"}]}, "lo" : %s , "acc":"%s","when":"%s", "uuid":"%s","la":%s}\t' % (
            _with_exponent(lon), acc, _civil(t), name(v), lat)
    return '{"uuid":"%s","when":"%s","la":%s,"lo":%s,"acc":%s,"speed":12.5}' % (name(v), _civil(t), lat, lon, acc)


def text(arr, kind, a=0, b=None, keep=None, bad_every=0):
    """Arrivals [a, b) as one chunk of text.  keep: a mask over the arrivals (others are left out).
    bad_every > 0: a malformed line in front of every arrival whose index is a multiple of it."""
    b = len(arr["vehicle"]) if b is None else b
    out = []
    for j in range(a, b):
        if keep is not None and not keep[j]:
            continue
        if bad_every and j % bad_every == 0:
            out.append(BAD[kind][(j // bad_every) % 3])
        out.append(message(arr, j, kind, j % 10 == 9))
    return ("\n".join(out) + "\n").encode() if out else b""
