"""The generic rule of separated-value trace lines (DESIGN.md rule 11) restated in plain Python:
strip, split, a regular expression for the number grammar, float(), calendar.timegm, math.ceil.
parse(chunks, fmt) returns what reporter_amd.engine.parse_lines_host returns, or raises Malformed
with the 1-based chunk and line of the first bad line."""
import calendar
import math
import re

import numpy as np

WS = b" \t\r\v\f"
NUMBER = re.compile(rb"[+-]?(\d+(\.\d*)?|\.\d+)([eE][+-]?\d+)?\Z")
INTEGER = re.compile(rb"[+-]?\d{1,18}\Z")


class Malformed(Exception):
    def __init__(self, chunk, line, why):
        Exception.__init__(self, "chunk %d line %d: %s" % (chunk, line, why))
        self.chunk, self.line = chunk, line


def number(field):
    if not NUMBER.match(field):
        raise ValueError("number")
    return float(field)


def civil_time(field):
    if len(field) != 19:
        raise ValueError("time")
    digits = [field[a:b] for a, b in ((0, 4), (5, 7), (8, 10), (11, 13), (14, 16), (17, 19))]
    if not all(re.match(rb"\d+\Z", d) for d in digits):
        raise ValueError("time")
    y, mo, d, h, mi, s = (int(x) for x in digits)
    if not (1 <= mo <= 12 and 1 <= d <= 31 and h <= 23 and mi <= 59 and s <= 60):
        raise ValueError("time")
    return calendar.timegm((y, mo, 1, 0, 0, 0)) + (d - 1) * 86400 + h * 3600 + mi * 60 + s


def line(text, fmt):
    """None for a blank line, "outside" for a point outside the box, else (id, time, lat, lon, acc)."""
    text = text.strip(WS)
    if not text:
        return None
    fields = text.split(fmt.sep)
    need = max(fmt.uuid_col, fmt.time_col, fmt.lat_col, fmt.lon_col, fmt.acc_col)
    if len(fields) <= need:
        raise ValueError("too few fields")
    get = lambda c: fields[c].strip(WS)
    lat = number(get(fmt.lat_col))
    lon = number(get(fmt.lon_col))
    b = fmt.bbox
    if b is not None and (lat < b[0] or lat > b[2] or lon < b[1] or lon > b[3]):
        return "outside"
    uid = get(fmt.uuid_col)
    if not 1 <= len(uid) <= 4096:
        raise ValueError("id")
    if fmt.time_format == 1:
        tm = civil_time(get(fmt.time_col))
    else:
        if not INTEGER.match(get(fmt.time_col)):
            raise ValueError("time")
        tm = int(get(fmt.time_col))
    acc = -1.0
    if fmt.acc_col >= 0:
        acc = math.ceil(number(get(fmt.acc_col)))
        if fmt.accuracy_cap > 0:
            acc = min(acc, fmt.accuracy_cap)
    return uid, float(tm), np.float32(lat), np.float32(lon), np.float32(acc)


def parse(chunks, fmt):
    ids, tm, lat, lon, acc = [], [], [], [], []
    table = {}
    info = dict(lines=0, blank=0, outside=0)
    for c, chunk in enumerate(chunks):
        chunk = bytes(chunk)
        lines = chunk.split(b"\n")
        if lines[-1] == b"":
            lines.pop()   # the text after the final newline is no line
        for k, text in enumerate(lines):
            try:
                r = line(text, fmt)
            except ValueError as e:
                raise Malformed(c + 1, k + 1, str(e))
            info["lines"] += 1
            if r is None:
                info["blank"] += 1
            elif r == "outside":
                info["outside"] += 1
            else:
                ids.append(table.setdefault(r[0], len(table)))
                tm.append(r[1]); lat.append(r[2]); lon.append(r[3]); acc.append(r[4])
    info["points"] = len(ids)
    info["vehicles"] = len(table)
    return dict(uuid=np.asarray(ids, np.uint32), time=np.asarray(tm, np.float64), lon=np.asarray(lon, np.float32),
                lat=np.asarray(lat, np.float32), accuracy=np.asarray(acc, np.float32),
                names=[k.decode("utf-8", "replace") for k in table], info=info)
