"""The generic rule of stream messages (DESIGN.md §3 rule 14) restated in plain Python: Python's
json for the object, float(), int(), calendar.timegm (through lines_ref), math.ceil; a dict for the
vehicle directory.  parse(chunks, fmt, strict) returns what reporter_amd.engine.parse_messages_host
returns, or (strict) raises Malformed with the text "chunk <c> line <l>: <reason>".  `fmt` is an
engine.MessageFormat (or anything with its kind, line and keys)."""
import json
import json.decoder
import math
import re

import numpy as np

import lines_ref
from lines_ref import WS, Malformed

JSON_WS = " \t\r"
INTEGER = re.compile(rb"[+-]?\d{1,18}\Z")
INT_TOKEN = re.compile(r"-?\d+\Z")
TIME0 = "malformed time (an integer of at most 18 digits)"
TIME1 = "malformed time (YYYY-MM-DD HH:MM:SS)"


class Bad(Exception):
    pass


def _number(field, why):
    try:
        return lines_ref.number(field)
    except ValueError:
        raise Bad(why)


def _finish(fmt, lat, lon, get_id, get_time, get_acc):
    """Rule 11's order behind lat and lon: the box, the id, the time, the accuracy."""
    b = fmt.bbox
    if b is not None and (lat < b[0] or lat > b[2] or lon < b[1] or lon > b[3]):
        return "outside"
    uid = get_id()
    tm = get_time()
    acc = get_acc()
    if acc is not None:
        acc = math.ceil(acc)
        if fmt.accuracy_cap > 0:
            acc = min(acc, fmt.accuracy_cap)
    return uid, float(tm), np.float32(lat), np.float32(lon), np.float32(-1.0 if acc is None else acc)


def _check_id(uid):
    if len(uid) == 0:
        raise Bad("empty vehicle id")
    if len(uid) > 4096:
        raise Bad("vehicle id longer than 4096 bytes")
    return uid


def _int_time(field):
    if not INTEGER.match(field):
        raise Bad(TIME0)
    return int(field)


def _civil(field):
    try:
        return lines_ref.civil_time(field)
    except ValueError:
        raise Bad(TIME1)


def sv_line(text, fmt):
    """Rule 11's line with the reader's reasons: None (blank), "outside" or (id, time, lat, lon, acc)."""
    text = text.strip(WS)
    if not text:
        return None
    fields = text.split(fmt.sep)
    if len(fields) <= max(fmt.uuid_col, fmt.time_col, fmt.lat_col, fmt.lon_col, fmt.acc_col):
        raise Bad("too few fields")
    get = lambda c: fields[c].strip(WS)
    lat = _number(get(fmt.lat_col), "malformed latitude")
    lon = _number(get(fmt.lon_col), "malformed longitude")
    return _finish(fmt, lat, lon, lambda: _check_id(get(fmt.uuid_col)),
                   lambda: _civil(get(fmt.time_col)) if fmt.time_format == 1 else _int_time(get(fmt.time_col)),
                   lambda: _number(get(fmt.acc_col), "malformed accuracy") if fmt.acc_col >= 0 else None)


def _no_constant(name):
    raise ValueError("NaN and Infinity are not JSON")


# (integer tokens as floats too: the rule takes a number node's double, and `-0` keeps its sign)
_DECODER = json.JSONDecoder(parse_constant=_no_constant, parse_int=float)


def _members(s):
    """(key, value, raw value text) of the top-level members of the object text `s`, in order."""
    out = []
    skip = lambda i: next((k for k in range(i, len(s)) if s[k] not in JSON_WS), len(s))
    i = skip(skip(0) + 1)   # behind '{'
    while s[i] == '"':
        key, i = json.decoder.scanstring(s, i + 1)
        i = skip(skip(i) + 1)   # behind ':'
        v, e = _DECODER.raw_decode(s, i)
        out.append((key, v, s[i:e]))
        i = skip(e)
        if s[i] != ",":
            break
        i = skip(i + 1)
    return out


def json_line(text, mf):
    fmt = mf.line
    text = text.strip(WS)
    if not text:
        return None
    s = text.decode("latin-1")   # byte for byte
    try:
        if "\0" in s or "\v" in s or "\f" in s:
            raise ValueError("not JSON whitespace")
        root = _DECODER.decode(s)
    except ValueError:
        raise Bad("invalid JSON")
    if not isinstance(root, dict):
        raise Bad("not a JSON object")
    node = {}
    for key, v, raw in _members(s):
        node[key] = (v, raw)   # of a repeated key the last wins
    keys = [k.decode("latin-1") for k in mf.keys]
    used = keys if keys[4] else keys[:4]
    if any(k not in node for k in used):
        raise Bad("missing key")

    def number(k, why):
        v = node[k][0]
        if isinstance(v, bool) or v is None:
            raise Bad(why)
        if isinstance(v, (int, float)):
            return float(v)
        if isinstance(v, str):
            return _number(v.encode("latin-1").strip(WS), why)
        raise Bad(why)

    def get_id():
        v, raw = node[keys[0]]
        if isinstance(v, str):
            if "\\" in raw:
                raise Bad("malformed vehicle id")
            return _check_id(raw[1:-1].encode("latin-1"))
        if isinstance(v, float) and INT_TOKEN.match(raw):
            return _check_id(raw.encode("latin-1"))
        raise Bad("malformed vehicle id")

    def get_time():
        v = node[keys[3]][0]
        if fmt.time_format == 1:
            if not isinstance(v, str):
                raise Bad(TIME1)
            return _civil(v.encode("latin-1"))
        if isinstance(v, bool) or v is None:
            raise Bad(TIME0)
        if isinstance(v, (int, float)):
            if not abs(v) < 2.0 ** 53:
                raise Bad(TIME0)
            return math.trunc(v)
        if isinstance(v, str):
            return _int_time(v.encode("latin-1").strip(WS))
        raise Bad(TIME0)

    lat = number(keys[1], "malformed latitude")
    lon = number(keys[2], "malformed longitude")
    return _finish(fmt, lat, lon, get_id, get_time, lambda: number(keys[4], "malformed accuracy") if keys[4] else None)


def message(text, mf):
    return json_line(text, mf) if mf.kind == 1 else sv_line(text, mf.line)


def parse(chunks, mf, strict=False):
    ids, tm, lat, lon, acc, names = [], [], [], [], [], []
    table = {}
    info = dict(lines=0, blank=0, outside=0, dropped=0)
    dropped = []
    for c, chunk in enumerate(chunks):
        lines = bytes(chunk).split(b"\n")
        if lines[-1] == b"":
            lines.pop()   # the text after the final newline is no line
        for k, text in enumerate(lines):
            info["lines"] += 1
            try:
                r = message(text, mf)
            except Bad as e:
                if strict:
                    raise Malformed(c + 1, k + 1, str(e))
                info["dropped"] += 1
                if len(dropped) < 64:
                    dropped.append((c + 1, k + 1, str(e)))
                continue
            if r is None:
                info["blank"] += 1
            elif r == "outside":
                info["outside"] += 1
            else:
                ids.append(table.setdefault(r[0], len(table)))
                names.append(r[0])
                tm.append(r[1]); lat.append(r[2]); lon.append(r[3]); acc.append(r[4])
    info["points"] = len(ids)
    info["vehicles"] = len(table)
    return dict(uuid=np.asarray(ids, np.uint32), time=np.asarray(tm, np.float64), lon=np.asarray(lon, np.float32),
                lat=np.asarray(lat, np.float32), accuracy=np.asarray(acc, np.float32),
                names=[k.decode("utf-8", "replace") for k in table], point_names=names, info=info, dropped=dropped)


class Directory:
    """The sequential model of the vehicle directory: a dict from id bytes to the next index."""

    def __init__(self, max_vehicles):
        self.max_vehicles = max_vehicles
        self.table = {}

    def assign(self, point_names):
        """The index of every point of one call; "directory full" leaves the directory as it was."""
        t = dict(self.table)
        out = [t.setdefault(n, len(t)) for n in point_names]
        if len(t) > self.max_vehicles:
            raise RuntimeError("directory full")
        self.table = t
        return np.asarray(out, np.uint32)

    def names(self):
        return [k.decode("utf-8", "replace") for k in self.table]
