"""Batched array API over the HIP engine (rm_engine / rm_runner of the C-ABI).

This is the high-throughput path the bench and the batch pipeline use: traces
go in as flat numpy arrays (CSR offsets per trace), every stage runs on the GPU,
and stage outputs can be downloaded for parity checks.  Requires a GPU.
"""
import ctypes as C
import os

import numpy as np

from . import _lib

SEGMENT_DTYPE = np.dtype([
    ("segment_id", "<u8"), ("start_time", "<f8"), ("end_time", "<f8"), ("length", "<i4"),
    ("queue_length", "<i4"), ("flags", "<u4"), ("begin_shape_index", "<u4"), ("end_shape_index", "<u4"),
    ("seg_dense", "<u4"), ("way_first", "<u4"), ("way_last", "<u4")])
assert SEGMENT_DTYPE.itemsize == 56

REPORT_DTYPE = np.dtype([
    ("id", "<u8"), ("next_id", "<u8"), ("t0", "<f8"), ("t1", "<f8"), ("length", "<i4"),
    ("queue_length", "<i4"), ("seg_dense", "<u4"), ("pad", "<u4")])
assert REPORT_DTYPE.itemsize == 48

STATS_DTYPE = np.dtype([
    ("successful_count", "<i4"), ("unreported_count", "<i4"), ("successful_length_m", "<i4"),
    ("unreported_length_m", "<i4"), ("discontinuities", "<i4"), ("invalid_speeds", "<i4"),
    ("invalid_times", "<i4"), ("unassociated", "<i4"), ("shape_used", "<i4"), ("n_reports", "<i4")])
assert STATS_DTYPE.itemsize == 40

# one matched point (rm_matched_point): type 0 unmatched, 1 matched (a state), 2 interpolated
MATCHED_POINT_DTYPE = np.dtype([
    ("lon", "<f4"), ("lat", "<f4"), ("sq", "<f4"), ("edge", "<u4"), ("off_cm", "<u4"), ("way", "<u4"),
    ("type", "<u4"), ("route_cm", "<u4")])
assert MATCHED_POINT_DTYPE.itemsize == 32

# one matched edge (rm_matched_edge): a visit of a directed edge by a matched chain; flags bit 0
# internal, bit 1 the edge has an OSMLR segment, bit 2 first visit of its chain
MATCHED_EDGE_DTYPE = np.dtype([
    ("edge", "<u4"), ("way", "<u4"), ("b_cm", "<u4"), ("e_cm", "<u4"), ("t_enter", "<f8"), ("t_exit", "<f8"),
    ("begin_point", "<u4"), ("end_point", "<u4"), ("shape_begin", "<u4"), ("shape_end", "<u4"),
    ("seg_dense", "<u4"), ("seg_off_cm", "<u4"), ("flags", "<u4"), ("len_cm", "<u4")])
assert MATCHED_EDGE_DTYPE.itemsize == 64

OPTIONS_DTYPE = np.dtype([
    ("mode", "<i4"), ("sigma_z", "<f4"), ("beta", "<f4"), ("search_radius", "<f4"), ("gps_accuracy", "<f4"),
    ("breakage_distance", "<f4"), ("interpolation_distance", "<f4"), ("max_route_distance_factor", "<f4"),
    ("max_route_time_factor", "<f4"), ("turn_penalty_factor", "<f4")])
assert OPTIONS_DTYPE.itemsize == 40

MAX_CAND = 16
INVALID_SEGMENT_ID = 0x3FFFFFFFFFFF  # Segment.java:16, simple_reporter.py:43


def default_options(n=1, **over):
    o = _lib.RmOptions()
    _lib.lib().rm_default_options(C.byref(o))
    a = np.zeros(n, OPTIONS_DTYPE)
    for name, _ in _lib.RmOptions._fields_:
        a[name] = getattr(o, name)
    for k, v in over.items():
        a[k] = v
    return a


def levels_mask(levels):
    """bit (level+1) per level, as the kernels and the oracle expect."""
    m = 0
    for lv in levels:
        if 0 <= int(lv) <= 7:
            m |= 1 << (int(lv) + 1)
    return m


class Engine:
    """The road graph resident in one GPU's HBM."""

    def __init__(self, graph_path, device=0):
        self._h = _lib.lib().rm_engine_create(os.fsencode(graph_path), int(device))
        if not self._h:
            raise _lib.RmError(_lib.last_error())
        self.graph_path = graph_path
        self.device = device

    @property
    def n_segments(self):
        return int(_lib.lib().rm_engine_n_segments(self._h))

    def segment_ids(self):
        ids = np.empty(self.n_segments, np.uint64)
        _lib.check(_lib.lib().rm_engine_segment_ids(self._h, ids.ctypes.data))
        return ids

    def set_ball_radius(self, meters):
        """Radius of the route balls (K2 lookup tier; 0 disables it).  Call before the first run."""
        _lib.check(_lib.lib().rm_engine_set_ball_radius(self._h, float(meters)))

    def ball_stats(self, mode=0):
        out = np.zeros(6, np.float64)
        _lib.check(_lib.lib().rm_engine_ball_stats(self._h, int(mode), out.ctypes.data))
        d = dict(zip(("radius_m", "keys", "entries", "nodes_without_table", "build_ms"), out[:5].tolist()))
        d["built_on_gpu"] = bool(out[5])
        return d

    def turn_rows(self):
        """Turn rows built so far (rule 3b): {mode name: build ms}."""
        mask = C.c_uint32(0)
        ms = np.zeros(5, np.float64)
        _lib.check(_lib.lib().rm_engine_turn_rows(self._h, C.byref(mask), ms.ctypes.data))
        names = ("auto", "bus", "motor_scooter", "bicycle", "pedestrian")
        return {names[m]: float(ms[m]) for m in range(5) if (mask.value >> m) & 1}

    def grid_split(self):
        """K1 grid refinement f (each graph-file cell split f x f)."""
        out = np.zeros(1, np.uint32)
        _lib.check(_lib.lib().rm_engine_grid_split(self._h, out.ctypes.data))
        return int(out[0])

    def grid_alt(self):
        """K1's second grid: (split f, batch radius in m from which it is used); (0, 0) if none."""
        f = np.zeros(1, np.uint32)
        r = np.zeros(1, np.float32)
        _lib.check(_lib.lib().rm_engine_grid_alt(self._h, f.ctypes.data, r.ctypes.data))
        return int(f[0]), float(r[0])

    def ball_lookup(self, mode, from_nodes, roads, preds=False):
        """Keys (n, 2) from each node to the two endpoints of each road through the engine's
        device tables of `mode` (all-ones outside the ball / without a table); with preds, also
        the rows' canonical predecessor indices (n, 2) (7: none stored)."""
        f = _c(from_nodes, np.uint32)
        r = _c(roads, np.uint32)
        keys = np.empty((len(f), 2), np.uint64)
        pr = np.empty((len(f), 2), np.uint8)
        _lib.check(_lib.lib().rm_engine_ball_lookup(self._h, int(mode), len(f), f.ctypes.data, r.ctypes.data,
                                                    keys.ctypes.data, pr.ctypes.data if preds else None))
        return (keys, pr) if preds else keys

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().rm_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


def _c(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


LINES_INFO = ("lines", "blank", "outside", "points", "vehicles", "host_lines", "ids_on_host")
DATE_PATTERN = "yyyy-MM-dd HH:mm:ss"


def time_pattern_id(pattern):
    """Compile and register a date pattern (rm_time_pattern; DESIGN.md §3 rule 18): the id that
    rm_line_format.time_format takes, the same for the same text.  ValueError with the compiler's
    message for a pattern that is not read."""
    text = pattern.encode() if isinstance(pattern, str) else bytes(pattern)
    err = C.create_string_buffer(256)
    pid = _lib.lib().rm_time_pattern(text, err, 256)
    if pid < 0:
        raise ValueError("time pattern %r: %s" % (text.decode("utf-8", "replace"), err.value.decode("utf-8", "replace")))
    return int(pid)


def parse_time(pattern, text):
    """One time text under one date pattern, on the host (rm_time_pattern_parse): the instant in
    whole seconds since 1970 UTC, or None for a text the pattern does not read."""
    pid = time_pattern_id(pattern)
    text = text.encode() if isinstance(text, str) else bytes(text)
    out = C.c_double(0.0)
    rc = _lib.lib().rm_time_pattern_parse(pid, text, len(text), C.byref(out))
    if rc == 2:
        raise _lib.RmError("time pattern id %d is not registered" % pid)
    return None if rc else float(out.value)


class LineFormat:
    """Layout of separated-value trace lines (rm_line_format).  The default is the trace files'
    ``uuid,time,lat,lon,accuracy`` (reference py/simple_reporter.py:113).  `time_pattern`: a date
    pattern (DESIGN.md §3 rule 18) that reads the time column, in place of a time_format; it is
    compiled here (ValueError with the compiler's message) and its id goes into the C struct."""

    def __init__(self, sep=b",", uuid_col=0, time_col=1, lat_col=2, lon_col=3, acc_col=4, time_format=0, accuracy_cap=0,
                 bbox=None, time_pattern=None):
        sep = sep.encode() if isinstance(sep, str) else bytes(sep)
        if len(sep) != 1:
            raise ValueError("the separator must be one byte")
        if bbox is not None and len(bbox) != 4:
            raise ValueError("bbox is min_lat, min_lon, max_lat, max_lon")
        self.sep, self.uuid_col, self.time_col, self.lat_col, self.lon_col = sep, int(uuid_col), int(time_col), int(lat_col), int(lon_col)
        self.acc_col, self.time_format, self.accuracy_cap = int(acc_col), int(time_format), int(accuracy_cap)
        self.bbox = None if bbox is None else tuple(float(x) for x in bbox)
        self.time_pattern = None
        if time_pattern is not None:
            if self.time_format != 0:
                raise ValueError("time_pattern stands in place of a time_format: give one of them")
            self.time_pattern = time_pattern.decode() if isinstance(time_pattern, bytes) else str(time_pattern)
            time_pattern_id(self.time_pattern)

    @classmethod
    def from_spec(cls, spec, **kw):
        """A formatter string of the reference (Formatter.java:36-51), e.g.
        ``,sv,\\|,1,9,10,0,5,yyyy-MM-dd HH:mm:ss``: the first character splits the rest into type,
        separator (one byte, optionally backslash-escaped), the uuid, lat, lon, time and accuracy
        columns, and an optional date pattern: yyyy-MM-dd HH:mm:ss is time_format 1, any other is
        compiled (rule 18)."""
        if len(spec) < 2:
            raise ValueError("empty formatter spec")
        args = spec[1:].split(spec[0])
        if args[0] == "json":
            raise ValueError("json formatters are not read here (separated values only)")
        if args[0] != "sv":
            raise ValueError("unsupported raw format parser: %r" % args[0])
        if len(args) < 7:
            raise ValueError("sv formatter needs separator, uuid, lat, lon, time and accuracy columns")
        sep = args[1][1:] if len(args[1]) == 2 and args[1][0] == "\\" else args[1]
        if len(sep.encode()) != 1:
            raise ValueError("the separator must be one byte")
        try:
            uuid, lat, lon, tm, acc = (int(a) for a in args[2:7])
        except ValueError:
            raise ValueError("sv formatter columns must be integers")
        pattern = args[7] if len(args) > 7 else None
        if pattern not in (None, DATE_PATTERN):
            return cls(sep, uuid, tm, lat, lon, acc, 0, time_pattern=pattern, **kw)
        return cls(sep, uuid, tm, lat, lon, acc, 1 if pattern else 0, **kw)

    def _c(self):
        f = _lib.RmLineFormat()
        _lib.lib().rm_default_line_format(C.byref(f))
        f.sep = self.sep[0]
        f.uuid_col, f.time_col, f.lat_col, f.lon_col, f.acc_col = self.uuid_col, self.time_col, self.lat_col, self.lon_col, self.acc_col
        f.time_format, f.accuracy_cap = self.time_format, self.accuracy_cap
        if self.time_pattern is not None:
            f.time_format = time_pattern_id(self.time_pattern)
        f.use_bbox = 0 if self.bbox is None else 1
        for k in range(4):
            f.bbox[k] = 0.0 if self.bbox is None else self.bbox[k]
        return f


def _chunk_views(chunks):
    """uint8 views of the chunks (no copy of bytes, memoryview or mmap objects)."""
    out = []
    for ch in chunks:
        a = _c(ch, np.uint8).reshape(-1) if isinstance(ch, np.ndarray) else np.frombuffer(ch, np.uint8)
        out.append(a)
    return out


def _lines_desc(chunks, fmt, inactivity, opts):
    views = _chunk_views(chunks)
    n = len(views)
    data = (C.c_void_p * max(n, 1))(*[v.ctypes.data if len(v) else None for v in views])
    lens = (C.c_uint64 * max(n, 1))(*[len(v) for v in views])
    opts = default_options(1) if opts is None else _c(opts, OPTIONS_DTYPE)
    d = _lib.RmLinesDesc(n, C.cast(data, C.c_void_p), C.cast(lens, C.c_void_p), (fmt or LineFormat())._c(),
                         float(inactivity), len(opts), opts.ctypes.data)
    return d, (views, data, lens, opts)


def _names(chunks, chunk, off, ln):
    views = _chunk_views(chunks)
    return [views[int(c)][int(o):int(o) + int(n)].tobytes().decode("utf-8", "replace") for c, o, n in zip(chunk, off, ln)]


def parse_lines_host(chunks, fmt=None):
    """The generic line rule over `chunks` on the host (no GPU): dict(uuid, time, lon, lat,
    accuracy, names, info), the points in input order and the vehicles in first-seen order."""
    d, keep = _lines_desc(chunks, fmt, 120.0, None)
    info = (C.c_uint64 * 7)()
    err = C.create_string_buffer(512)
    L = _lib.lib()
    if L.rm_lines_parse_host(C.byref(d), info, None, None, None, None, None, None, None, None, err, 512) != 0:
        raise _lib.RmError(err.value.decode("utf-8", "replace"))
    n, nv = int(info[3]), int(info[4])
    uuid = np.empty(n, np.uint32)
    time = np.empty(n, np.float64)
    lon, lat, acc = (np.empty(n, np.float32) for _ in range(3))
    chunk = np.empty(nv, np.uint32)
    off = np.empty(nv, np.uint64)
    ln = np.empty(nv, np.uint32)
    if L.rm_lines_parse_host(C.byref(d), info, uuid.ctypes.data, time.ctypes.data, lon.ctypes.data, lat.ctypes.data,
                             acc.ctypes.data, chunk.ctypes.data, off.ctypes.data, ln.ctypes.data, err, 512) != 0:
        raise _lib.RmError(err.value.decode("utf-8", "replace"))
    return dict(uuid=uuid, time=time, lon=lon, lat=lat, accuracy=acc, names=_names(chunks, chunk, off, ln),
                info=dict(zip(LINES_INFO, (int(x) for x in info))))


INPUT_CODINGS = ("plain", "gzip", "auto")
INFLATE_INFO = ("members", "bytes_in", "bytes_out", "second_pass")


def inflate_status_text(status):
    return _lib.lib().rm_inflate_status_text(int(status)).decode()


def _inflate(chunks, device):
    views = _chunk_views(chunks)
    n = len(views)
    data = (C.c_void_p * max(n, 1))(*[v.ctypes.data if len(v) else None for v in views])
    lens = (C.c_uint64 * max(n, 1))(*[len(v) for v in views])
    status = np.zeros(n, np.uint32)
    out_len = np.zeros(n, np.uint64)
    blob, blen = C.c_void_p(), C.c_size_t()
    L = _lib.lib()
    if device is None:
        _lib.check(L.rm_inflate_host(n, data, lens, status.ctypes.data, out_len.ctypes.data, C.byref(blob), C.byref(blen)))
    else:
        _lib.check(L.rm_inflate(int(device), n, data, lens, status.ctypes.data, out_len.ctypes.data, C.byref(blob),
                                C.byref(blen)))
    try:
        flat = C.string_at(blob, blen.value)
    finally:
        L.rm_free(blob)
    out, at = [], 0
    for c in range(n):
        m = int(out_len[c])
        out.append(flat[at:at + m] if status[c] == 0 else None)
        at += m
    return out, [int(s) for s in status]


def inflate(chunks, device=0):
    """Gzip chunks (DESIGN.md §3 rule 20) inflated and checked on the GPU, a wave per chunk:
    (list of bytes, None for a bad chunk; rule 20's status per chunk).  inflate_last() has the
    call's counts and times."""
    return _inflate(chunks, device)


def inflate_host(chunks):
    """The same decoder core on the host pool (no GPU)."""
    return _inflate(chunks, None)


def inflate_last():
    """Of the calling thread's last inflate / inflate_host call (rm_inflate_last): members,
    bytes_in, bytes_out, second_pass (chunks the device inflated twice: their slot was too small)
    and ms (inflate with the CRC, 0, gather)."""
    info = (C.c_uint64 * 4)()
    ms = (C.c_double * 3)()
    _lib.lib().rm_inflate_last(info, ms)
    return dict(zip(INFLATE_INFO, (int(x) for x in info)), ms=tuple(float(x) for x in ms))


MESSAGES_INFO = LINES_INFO + ("dropped",)
MESSAGE_KEYS = ("id", "lat", "lon", "time", "accuracy")


class MessageFormat:
    """Layout of raw stream messages (rm_message_format; DESIGN.md §3 rule 14): kind 0, separated
    values read by `line` (a LineFormat); kind 1, one JSON object per line whose members `keys`
    (id, lat, lon, time, accuracy; an empty accuracy key: none) hold the values, with `line`'s
    time_format, accuracy_cap and bbox."""

    def __init__(self, kind=0, line=None, keys=("id", "latitude", "longitude", "timestamp", "accuracy")):
        if kind not in (0, 1):
            raise ValueError("kind is 0 (separated values) or 1 (JSON)")
        keys = tuple(k.encode() if isinstance(k, str) else bytes(k) for k in keys)
        if len(keys) != 5:
            raise ValueError("keys are id, lat, lon, time, accuracy")
        if kind == 1:
            if any(len(k) > 31 for k in keys):
                raise ValueError("a key is longer than 31 bytes")
            if any(len(k) == 0 for k in keys[:4]):
                raise ValueError("the id, lat, lon and time keys cannot be empty")
            if any(c in b'"\\' or c < 0x20 for k in keys for c in k):
                raise ValueError("a key holds a quote, a backslash or a control byte")
            used = [k for k in keys if k]
            if len(set(used)) != len(used):
                raise ValueError("two keys are equal")
        self.kind, self.line, self.keys = int(kind), line or LineFormat(), keys

    @classmethod
    def from_spec(cls, spec, **kw):
        """Either formatter string of the reference (Formatter.java:36-51): the separated-value form
        LineFormat.from_spec reads, or ``@json@id@lat@lon@time@accuracy[@yyyy-MM-dd'T'HH:mm:ssZZ]`` (the
        first character splits the rest into type, the five keys and an optional date pattern, read
        as LineFormat.from_spec reads it)."""
        if len(spec) < 2:
            raise ValueError("empty formatter spec")
        args = spec[1:].split(spec[0])
        if args[0] == "sv":
            return cls(0, LineFormat.from_spec(spec, **kw))
        if args[0] != "json":
            raise ValueError("unsupported raw format parser: %r" % args[0])
        if len(args) < 6:
            raise ValueError("json formatter needs the id, lat, lon, time and accuracy keys")
        pattern = args[6] if len(args) > 6 else None
        if pattern not in (None, DATE_PATTERN):
            return cls(1, LineFormat(time_pattern=pattern, **kw), args[1:6])
        return cls(1, LineFormat(time_format=1 if pattern else 0, **kw), args[1:6])

    def _c(self):
        f = _lib.RmMessageFormat()
        _lib.lib().rm_default_message_format(C.byref(f))
        f.kind = self.kind
        f.line = self.line._c()
        for i, k in enumerate(self.keys):
            f.key[i].value = k if self.kind == 1 else b""
        return f


def _messages_desc(chunks, fmt, strict, stamp_ms):
    views = _chunk_views(chunks)
    n = len(views)
    data = (C.c_void_p * max(n, 1))(*[v.ctypes.data if len(v) else None for v in views])
    lens = (C.c_uint64 * max(n, 1))(*[len(v) for v in views])
    fmt = fmt or MessageFormat()
    if isinstance(fmt, LineFormat):
        fmt = MessageFormat(0, fmt)
    d = _lib.RmMessagesDesc(n, C.cast(data, C.c_void_p), C.cast(lens, C.c_void_p), fmt._c(), 1 if strict else 0,
                            0 if stamp_ms is None else 1, 0 if stamp_ms is None else int(stamp_ms))
    return d, (views, data, lens)


def _dropped(n, chunk, line, reasons):
    why = reasons.raw.split(b"\0")
    return [(int(chunk[k]), int(line[k]), why[k].decode()) for k in range(int(n.value))]


def parse_messages_host(chunks, fmt=None, strict=False):
    """Rule 14's generic rule over `chunks` on the host (no GPU): parse_lines_host's dict with
    info["dropped"] and `dropped`, the first (at most 64) malformed messages of a tolerant call as
    (chunk, line, reason), both 1-based.  A strict call raises on the first one instead."""
    d, keep = _messages_desc(chunks, fmt, strict, None)
    info = (C.c_uint64 * 8)()
    err = C.create_string_buffer(512)
    L = _lib.lib()
    if L.rm_messages_parse_host(C.byref(d), info, None, None, None, None, None, None, None, None, None, None, None, None, 0,
                                err, 512) != 0:
        raise _lib.RmError(err.value.decode("utf-8", "replace"))
    n, nv = int(info[3]), int(info[4])
    uuid = np.empty(n, np.uint32)
    time = np.empty(n, np.float64)
    lon, lat, acc = (np.empty(n, np.float32) for _ in range(3))
    chunk = np.empty(nv, np.uint32)
    off = np.empty(nv, np.uint64)
    ln = np.empty(nv, np.uint32)
    nd = C.c_uint32(0)
    dchunk = (C.c_uint32 * 64)()
    dline = (C.c_uint64 * 96)()
    reasons = C.create_string_buffer(64 * 96)
    if L.rm_messages_parse_host(C.byref(d), info, uuid.ctypes.data, time.ctypes.data, lon.ctypes.data, lat.ctypes.data,
                                acc.ctypes.data, chunk.ctypes.data, off.ctypes.data, ln.ctypes.data, C.byref(nd),
                                C.addressof(dchunk), C.addressof(dline), C.addressof(reasons), 64 * 96, err, 512) != 0:
        raise _lib.RmError(err.value.decode("utf-8", "replace"))
    return dict(uuid=uuid, time=time, lon=lon, lat=lat, accuracy=acc, names=_names(chunks, chunk, off, ln),
                info=dict(zip(MESSAGES_INFO, (int(x) for x in info))), dropped=_dropped(nd, dchunk, dline, reasons))


class VehicleDirectory:
    """The map from vehicle id bytes to a dense index that holds for a whole stream, kept on the GPU
    (rm_directory_*; DESIGN.md §3 rule 14): indices in first-seen order over every call's kept points."""

    def __init__(self, max_vehicles, device=0):
        self.max_vehicles = int(max_vehicles)
        self._h = _lib.lib().rm_directory_create(int(device), self.max_vehicles)
        if not self._h:
            raise _lib.RmError(_lib.last_error())

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().rm_directory_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    @property
    def size(self):
        n = C.c_uint32(0)
        _lib.check(_lib.lib().rm_directory_size(self._h, C.byref(n)))
        return int(n.value)

    def names(self, first=0, n=None):
        """The names of vehicles [first, first + n) (default: all), in index order."""
        n = self.size - first if n is None else int(n)
        nb = C.c_uint64(0)
        off = np.zeros(n + 1, np.uint64)
        _lib.check(_lib.lib().rm_directory_names(self._h, int(first), n, off.ctypes.data, None, C.byref(nb)))
        raw = np.zeros(max(int(nb.value), 1), np.uint8)
        _lib.check(_lib.lib().rm_directory_names(self._h, int(first), n, off.ctypes.data, raw.ctypes.data, C.byref(nb)))
        b = raw.tobytes()
        return [b[int(off[k]):int(off[k + 1])].decode("utf-8", "replace") for k in range(n)]


class BatchMatcher:
    """One HIP stream + device workspace; runs whole batches of traces."""

    def __init__(self, engine):
        self.engine = engine
        self._h = _lib.lib().rm_runner_create(engine._h)
        if not self._h:
            raise _lib.RmError(_lib.last_error())
        self._keep = None

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().rm_runner_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    @staticmethod
    def run_params(threshold_sec=15.0, report_levels=(0, 1), transition_levels=(0, 1), hist_dev=None,
                   do_report=True, zero_hist=False, dur_dev=None):
        rp = _lib.RmRunParams()
        rp.threshold_sec = threshold_sec
        rp.report_mask = levels_mask(report_levels)
        rp.transition_mask = levels_mask(transition_levels)
        rp.hist_dev = hist_dev or None
        rp.do_report = 1 if do_report else 0
        rp.zero_hist = 1 if zero_hist else 0
        rp.dur_dev = dur_dev or None
        return rp

    def run(self, trace_off, lon, lat, time, accuracy=None, opts=None, trace_opt=None, **rp_kw):
        """Upload a batch and run every stage (blocks until done)."""
        trace_off = _c(trace_off, np.uint32)
        T = len(trace_off) - 1
        P = int(trace_off[-1])
        lon = _c(lon, np.float32)
        lat = _c(lat, np.float32)
        time = _c(time, np.float64)
        accuracy = _c(np.full(P, -1.0, np.float32) if accuracy is None else accuracy, np.float32)
        opts = default_options(1) if opts is None else _c(opts, OPTIONS_DTYPE)
        trace_opt = np.zeros(T, np.uint32) if trace_opt is None else _c(trace_opt, np.uint32)
        if not (len(lon) == len(lat) == len(time) == len(accuracy) == P):
            raise ValueError("point arrays must all have trace_off[-1] elements")
        if len(trace_opt) != T:
            raise ValueError("trace_opt must have one entry per trace")
        d = _lib.RmBatchDesc(T, trace_off.ctypes.data, lon.ctypes.data, lat.ctypes.data, time.ctypes.data,
                             accuracy.ctypes.data, len(opts), opts.ctypes.data, trace_opt.ctypes.data)
        self._keep = (trace_off, lon, lat, time, accuracy, opts, trace_opt)
        rp = self.run_params(**rp_kw)
        _lib.check(_lib.lib().rm_runner_run(self._h, C.byref(d), C.byref(rp)))
        return self

    def run_points(self, uuid, time, lon, lat, accuracy=None, inactivity=120.0, opts=None, uuid_opt=None, n_uuids=None,
                   **rp_kw):
        """Raw per-vehicle points (any order) -> device time sort + inactivity windows of
        >= 2 points (reference py/simple_reporter.py:137-164) -> every matching stage.
        `uuid` is a dense vehicle index per point.  Blocks until done."""
        uuid = _c(uuid, np.uint32)
        n = len(uuid)
        time = _c(time, np.float64)
        lon = _c(lon, np.float32)
        lat = _c(lat, np.float32)
        accuracy = None if accuracy is None else _c(accuracy, np.float32)
        if not (len(time) == len(lon) == len(lat) == n) or (accuracy is not None and len(accuracy) != n):
            raise ValueError("point arrays must have equal lengths")
        nu = int(n_uuids if n_uuids is not None else (int(uuid.max()) + 1 if n else 0))
        opts = default_options(1) if opts is None else _c(opts, OPTIONS_DTYPE)
        uuid_opt = None if uuid_opt is None else _c(uuid_opt, np.uint32)
        if uuid_opt is not None and len(uuid_opt) != nu:
            raise ValueError("uuid_opt must have one entry per vehicle")
        d = _lib.RmPointsDesc(n, uuid.ctypes.data, time.ctypes.data, lon.ctypes.data, lat.ctypes.data,
                              accuracy.ctypes.data if accuracy is not None else None, float(inactivity), nu, len(opts),
                              opts.ctypes.data, uuid_opt.ctypes.data if uuid_opt is not None else None)
        self._keep = (uuid, time, lon, lat, accuracy, opts, uuid_opt)
        rp = self.run_params(**rp_kw)
        _lib.check(_lib.lib().rm_runner_run_points(self._h, C.byref(d), C.byref(rp)))
        return self

    def run_lines(self, chunks, fmt=None, inactivity=120.0, opts=None, **rp_kw):
        """Trace-file text (one chunk per file: bytes, memoryview, mmap or uint8 arrays) -> lines
        parsed, vehicle ids numbered in first-seen order, inactivity windows and every matching
        stage, all on the device (DESIGN.md rule 11).  Every window takes opts[0].  A malformed
        line raises RuntimeError "chunk <c> line <l>: <reason>"."""
        d, keep = _lines_desc(chunks, fmt, inactivity, opts)
        self._keep = keep
        rp = self.run_params(**rp_kw)
        _lib.check(_lib.lib().rm_runner_run_lines(self._h, C.byref(d), C.byref(rp)))
        return self

    def parse_lines(self, chunks, fmt=None):
        """The parse and id stages of run_lines alone; returns the kept points in input order:
        dict(uuid, time, lon, lat, accuracy)."""
        d, keep = _lines_desc(chunks, fmt, 120.0, None)
        self._keep = keep
        _lib.check(_lib.lib().rm_runner_parse_lines(self._h, C.byref(d)))
        return self.line_points()

    def line_points(self):
        """The points of the last run_lines / parse_lines, in input order."""
        n = self.lines_info()["points"]
        uuid = np.empty(n, np.uint32)
        time = np.empty(n, np.float64)
        lon, lat, acc = (np.empty(n, np.float32) for _ in range(3))
        _lib.check(_lib.lib().rm_runner_get_line_points(self._h, uuid.ctypes.data, time.ctypes.data, lon.ctypes.data,
                                                        lat.ctypes.data, acc.ctypes.data))
        return dict(uuid=uuid, time=time, lon=lon, lat=lat, accuracy=acc)

    def lines_info(self):
        out = (C.c_uint64 * 7)()
        _lib.check(_lib.lib().rm_runner_lines_info(self._h, out))
        return dict(zip(LINES_INFO, (int(x) for x in out)))

    def vehicle_names(self, chunks=None):
        """Vehicle id strings of the last run_lines / parse_lines over `chunks`, by vehicle index.
        Without chunks the names are read back from the device text (gzip chunks: the caller does
        not hold the inflated text)."""
        n = self.lines_info()["vehicles"]
        chunk = np.empty(n, np.uint32)
        off = np.empty(n, np.uint64)
        ln = np.empty(n, np.uint32)
        _lib.check(_lib.lib().rm_runner_get_vehicles(self._h, chunk.ctypes.data, off.ctypes.data, ln.ctypes.data))
        if chunks is not None:
            return _names(chunks, chunk, off, ln)
        return [self.text(c, o, m).decode("utf-8", "replace") for c, o, m in zip(chunk, off, ln)]

    def text(self, chunk, off, length):
        """bytes [off, off + length) of chunk `chunk` of the last parse's text, from the device"""
        buf = C.create_string_buffer(max(int(length), 1))
        _lib.check(_lib.lib().rm_runner_get_text(self._h, int(chunk), int(off), int(length), buf))
        return buf.raw[:int(length)]

    def set_input_coding(self, coding="plain", skip_bad=False):
        """How run_lines, parse_lines and a VehicleSessions' push_messages over this matcher read
        their chunks from now on (DESIGN.md rule 20): "plain" (the default), "gzip" (every chunk
        is a sequence of gzip members, inflated and checked on the device), or "auto" (gzip where
        a chunk begins 1f 8b).  A bad chunk raises "chunk <c>: gzip: <reason>"; with skip_bad it
        counts as empty and chunk_status() names it."""
        _lib.check(_lib.lib().rm_runner_set_input_coding(self._h, INPUT_CODINGS.index(coding), 1 if skip_bad else 0))
        return self

    def chunk_status(self):
        """Rule 20's status of every chunk of this matcher's last parse (0: ok or plain), whichever
        call made it: run_lines, parse_lines or a VehicleSessions' push_messages."""
        k = C.c_uint32(0)
        _lib.check(_lib.lib().rm_runner_chunk_count(self._h, C.byref(k)))
        n = int(k.value)
        out = np.zeros(max(n, 1), np.uint32)
        _lib.check(_lib.lib().rm_runner_chunk_status(self._h, out.ctypes.data))
        return [int(s) for s in out[:n]]

    def inflate_info(self):
        out = (C.c_uint64 * 6)()
        _lib.check(_lib.lib().rm_runner_inflate_info(self._h, out))
        return dict(zip(("chunks", "members", "bytes_in", "bytes_out", "second_pass", "host_chunks"), (int(x) for x in out)))

    def inflate_ms(self):
        """Times (ms) of the last parse's gzip parts: inflate (with the CRC), crc (0: it is computed
        as the window is flushed), gather.  The compressed upload is lines_ms()'s upload."""
        out = (C.c_double * 3)()
        _lib.check(_lib.lib().rm_runner_inflate_time(self._h, out))
        return dict(zip(("inflate", "crc", "gather"), (float(x) for x in out)))

    def lines_ms(self):
        """Times (ms) of the last run_lines' parts: upload, parse (+ host lines), ids, windows."""
        out = (C.c_double * 4)()
        _lib.check(_lib.lib().rm_runner_lines_time(self._h, out))
        return dict(zip(("upload", "parse", "ids", "windows"), (float(x) for x in out)))

    def trace_uuid(self):
        """Vehicle index of every matched window of the last run_points."""
        out = np.empty(self.sizes()["traces"], np.uint32)
        _lib.check(_lib.lib().rm_runner_get_trace_uuid(self._h, out.ctypes.data))
        return out

    def batch(self):
        """The batch the last run matched (after run_points: the device-built windows)."""
        sz = self.sizes()
        P, T = sz["points"], sz["traces"]
        off = np.empty(T + 1, np.uint32)
        lon, lat, acc = (np.empty(P, np.float32) for _ in range(3))
        time = np.empty(P, np.float64)
        _lib.check(_lib.lib().rm_runner_get_batch(self._h, off.ctypes.data, lon.ctypes.data, lat.ctypes.data,
                                                  time.ctypes.data, acc.ctypes.data))
        return dict(trace_off=off, lon=lon, lat=lat, time=time, accuracy=acc)

    def tiles(self, quantisation=3600, privacy=2, source="smpl_rprt", mode="auto", comm=None):
        """Time tiles of the last run's reports: {"<start>_<end>/<level>/<index>": CSV text}
        exactly as the reference's report phase uploads them (py/simple_reporter.py:176-254).
        With a dist.Comm, rows of every rank are all-gathered and this rank's files returned."""
        tp = _lib.RmTileParams(int(quantisation), int(privacy), source.encode(), mode.encode())
        blob = C.c_void_p()
        n = C.c_size_t()
        _lib.check(_lib.lib().rm_runner_tiles(self._h, C.byref(tp), comm._h if comm is not None else None,
                                              C.byref(blob), C.byref(n)))
        try:
            raw = C.string_at(blob.value, n.value) if n.value else b""
        finally:
            _lib.lib().rm_free(blob)
        parts = raw.split(b"\0")
        return {parts[i].decode(): parts[i + 1].decode() for i in range(0, len(parts) - 1, 2)}

    def rerun(self, **rp_kw):
        """Run every stage again over the batch already in HBM."""
        rp = self.run_params(**rp_kw)
        _lib.check(_lib.lib().rm_runner_rerun(self._h, C.byref(rp)))

    def sizes(self):
        out = (C.c_uint64 * 10)()
        _lib.check(_lib.lib().rm_runner_sizes(self._h, out))
        return dict(zip(("points", "traces", "transitions", "path_edges", "segments", "reports", "routes_tier2",
                         "routes_tier3", "paths_tier2", "cand_tier2"), [int(x) for x in out]))

    def route_tiers(self):
        """Hand-overs of the last run: K2 ball tier -> search, register tier -> tier 2, tier 2 -> the
        LDS tiers (16-lane groups, then 512- and 4096-slot waves), wave -> global; the same for the
        path stage."""
        out = (C.c_uint64 * 10)()
        _lib.check(_lib.lib().rm_runner_route_tiers(self._h, out))
        return dict(zip(("ball_to_search", "lane_to_tier2", "tier2_to_wave", "paths_ball_to_search",
                         "wave_to_global", "paths_wave_to_global", "group_to_wave512", "paths_group_to_wave512",
                         "wave512_to_wave4096", "paths_wave512_to_wave4096"), [int(x) for x in out]))

    def run_stats(self):
        """Counters since creation: steady runs, steady runs gated off on the device and run again
        the ordinary way, and steady runs that left out the routes / path stage's hand-over tiers."""
        out = (C.c_uint64 * 4)()
        _lib.check(_lib.lib().rm_runner_run_stats(self._h, out))
        return dict(zip(("steady", "steady_rerun", "routes_tiers_skipped", "paths_tiers_skipped"),
                        [int(x) for x in out]))

    # ---- stage outputs (parity tests) ----
    def states(self):
        s = self.sizes()
        n_states = np.empty(s["traces"], np.uint32)
        orig = np.empty(s["points"], np.uint32)
        _lib.check(_lib.lib().rm_runner_get_states(self._h, n_states.ctypes.data, orig.ctypes.data))
        return n_states, orig

    def candidates(self):
        P = self.sizes()["points"]
        n = np.empty(P, np.uint8)
        road = np.empty(P * MAX_CAND, np.uint32)
        s = np.empty(P * MAX_CAND, np.uint32)
        sq = np.empty(P * MAX_CAND, np.float32)
        _lib.check(_lib.lib().rm_runner_get_candidates(self._h, n.ctypes.data, road.ctypes.data, s.ctypes.data,
                                                       sq.ctypes.data))
        return n, road.reshape(P, MAX_CAND), s.reshape(P, MAX_CAND), sq.reshape(P, MAX_CAND)

    def routes(self):
        sz = self.sizes()
        off = np.empty(sz["points"], np.uint32)
        gc = np.empty(sz["points"], np.float64)
        route = np.empty(max(sz["transitions"], 1), np.uint32)
        _lib.check(_lib.lib().rm_runner_get_routes(self._h, off.ctypes.data, gc.ctypes.data, route.ctypes.data))
        return off, gc, route[: sz["transitions"]]

    def route_terms(self):
        """With turn costs (DESIGN.md §3 rule 3b): every transition's distance term turn_m +
        |route_m - gc| (metres, inf when invalid) as the Viterbi adds it; None when the last run
        had no turn costs."""
        n = self.sizes()["transitions"]
        out = np.empty(max(n, 1), np.float64)
        present = C.c_int(0)
        _lib.check(_lib.lib().rm_runner_get_route_terms(self._h, out.ctypes.data, C.byref(present)))
        return out[:n] if present.value else None

    def viterbi(self):
        P = self.sizes()["points"]
        choice = np.empty(P, np.int8)
        cs = np.empty(P, np.uint8)
        _lib.check(_lib.lib().rm_runner_get_viterbi(self._h, choice.ctypes.data, cs.ctypes.data))
        return choice, cs

    def paths(self):
        sz = self.sizes()
        off = np.empty(sz["points"], np.uint32)
        cnt = np.empty(sz["points"], np.uint32)
        pool = np.empty(max(sz["path_edges"], 1), np.uint32)
        dist = np.empty(sz["points"], np.uint32)
        _lib.check(_lib.lib().rm_runner_get_paths(self._h, off.ctypes.data, cnt.ctypes.data, pool.ctypes.data,
                                                  dist.ctypes.data))
        return off, cnt, pool, dist

    def segments(self):
        sz = self.sizes()
        off = np.empty(sz["traces"] + 1, np.uint32)
        segs = np.empty(max(sz["segments"], 1), SEGMENT_DTYPE)
        _lib.check(_lib.lib().rm_runner_get_segments(self._h, off.ctypes.data, segs.ctypes.data))
        return off, segs[: sz["segments"]]

    def matched_points(self):
        """Where every input point of the last run ended up on the road (DESIGN.md §3 rule 9):
        one MATCHED_POINT_DTYPE record per point, in batch point order.  The stage runs on this
        call (kernel id "points"), not during run()."""
        out = np.empty(self.sizes()["points"], MATCHED_POINT_DTYPE)
        _lib.check(_lib.lib().rm_runner_get_matched_points(self._h, out.ctypes.data))
        return out

    def matched_edges(self):
        """Every edge visit of the last run with its times, and each trace's matched polyline
        (DESIGN.md §3 rule 10): (edge_off, edges, shape_off, shape).  Trace k's visits are
        edges[edge_off[k]:edge_off[k+1]] (MATCHED_EDGE_DTYPE), its vertices
        shape[shape_off[k]:shape_off[k+1]] ((lon, lat) rows, float32; a visit's shape_begin /
        shape_end index them).  The stage runs on this call, not during run()."""
        T = self.sizes()["traces"]
        tot = (C.c_uint64 * 2)()
        _lib.check(_lib.lib().rm_runner_matched_edges(self._h, tot))
        edge_off = np.zeros(T + 1, np.uint32)
        shape_off = np.zeros(T + 1, np.uint32)
        edges = np.empty(max(int(tot[0]), 1), MATCHED_EDGE_DTYPE)
        shape = np.empty((max(int(tot[1]), 1), 2), np.float32)
        _lib.check(_lib.lib().rm_runner_get_matched_edges(self._h, edge_off.ctypes.data, edges.ctypes.data,
                                                          shape_off.ctypes.data, shape.ctypes.data))
        return edge_off, edges[: int(tot[0])], shape_off, shape[: int(tot[1])]

    def matched_edges_ms(self):
        """Device time (ms) of the last matched_edges(): HIP events round its launches."""
        ms = C.c_double(0.0)
        _lib.check(_lib.lib().rm_runner_matched_edges_time(self._h, C.byref(ms)))
        return float(ms.value)

    def reports(self):
        sz = self.sizes()
        off = np.empty(sz["traces"] + 1, np.uint32)
        reps = np.empty(max(sz["reports"], 1), REPORT_DTYPE)
        stats = np.empty(sz["traces"], STATS_DTYPE)
        _lib.check(_lib.lib().rm_runner_get_reports(self._h, off.ctypes.data, reps.ctypes.data, stats.ctypes.data))
        return off, reps[: sz["reports"]], stats

    def set_isolation(self, on=True):
        """Per-trace failure isolation (rm_runner_set_isolation): a failing trace gets no output
        instead of failing the run; see trace_errors()."""
        _lib.check(_lib.lib().rm_runner_set_isolation(self._h, 1 if on else 0))

    def set_locality(self, mode):
        """Locality order of K1 / K2 / paths (rm_runner_set_locality): -1 engine default, 0 slot
        order, 1 sorted by region.  Results are identical either way."""
        _lib.check(_lib.lib().rm_runner_set_locality(self._h, int(mode)))

    def locality_used(self):
        v = C.c_int(0)
        _lib.check(_lib.lib().rm_runner_locality_used(self._h, C.byref(v)))
        return bool(v.value)

    def trace_errors(self):
        """Error bits per trace of the last run (1 candidates, 2 route search, 8 path rebuild)."""
        out = np.zeros(self.sizes()["traces"], np.uint32)
        _lib.check(_lib.lib().rm_runner_trace_errors(self._h, out.ctypes.data))
        return out

    # ---- timing ----
    def set_timing(self, on=True):
        _lib.check(_lib.lib().rm_runner_set_timing(self._h, 1 if on else 0))

    def set_timing_stages(self, names):
        """Time only the named stages (rm_kernel_name), e.g. ("routes",)."""
        n = _lib.lib().rm_num_kernels()
        idx = {_lib.lib().rm_kernel_name(i).decode(): i for i in range(n)}
        mask = 0
        for nm in names:
            mask |= 1 << idx[nm]
        _lib.check(_lib.lib().rm_runner_set_timing_mask(self._h, mask))

    def reset_times(self):
        _lib.check(_lib.lib().rm_runner_reset_times(self._h))

    def kernel_times(self):
        n = _lib.lib().rm_num_kernels()
        ms = np.zeros(n, np.float64)
        la = np.zeros(n, np.uint64)
        _lib.check(_lib.lib().rm_runner_kernel_times(self._h, ms.ctypes.data, la.ctypes.data, n))
        names = [_lib.lib().rm_kernel_name(i).decode() for i in range(n)]
        return {names[i]: (float(ms[i]), int(la[i])) for i in range(n)}


SESSION_REPORT_DTYPE = np.dtype(REPORT_DTYPE.descr + [("vehicle", "<u4"), ("window", "<u4")])
assert SESSION_REPORT_DTYPE.itemsize == 56

SESSION_WINDOW_DTYPE = np.dtype([
    ("vehicle", "<u4"), ("arrival", "<u4"), ("n_points", "<u4"), ("shape_used", "<i4"), ("n_reports", "<u4"),
    ("err", "<u4")])
assert SESSION_WINDOW_DTYPE.itemsize == 24

SESSION_CAPPED = 0x80000000   # SESSION_WINDOW_DTYPE err: cleared at max_vehicle_points, not matched
SESSION_COUNTS = ("arrivals", "triggers", "trims", "cleared", "failed", "forwarded", "invalid", "rounds")


class VehicleSessions:
    """The streaming batcher of the reference (BatchingProcessor.java, Batch.java) kept on the GPU
    beside a BatchMatcher (rm_session_*; DESIGN.md §3 rule 12).  push() takes arrivals as arrays,
    punctuate() evicts stale vehicles; reports() / windows() give the last call's output ordered by
    triggering arrival.  The matcher's batch is replaced by each round's windows."""

    def __init__(self, batch_matcher, n_vehicles, report_dist_m=None, report_count=None, report_time_s=None,
                 session_gap_ms=None, max_vehicle_points=0, opts=None, **rp_kw):
        self.matcher = batch_matcher
        self.n_vehicles = int(n_vehicles)
        p = _lib.RmSessionParams()
        _lib.lib().rm_default_session_params(C.byref(p))
        if report_dist_m is not None:
            p.report_dist_m = float(report_dist_m)
        if report_count is not None:
            p.report_count = int(report_count)
        if report_time_s is not None:
            p.report_time_s = float(report_time_s)
        if session_gap_ms is not None:
            p.session_gap_ms = int(session_gap_ms)
        p.max_vehicle_points = int(max_vehicle_points)
        if opts is not None:
            o = _c(opts, OPTIONS_DTYPE)
            if len(o) != 1:
                raise ValueError("a session takes one option set")
            for name, _ in _lib.RmOptions._fields_:
                setattr(p.opt, name, o[name][0].item())
        p.run = BatchMatcher.run_params(**rp_kw)
        self._h = _lib.lib().rm_session_create(batch_matcher._h, self.n_vehicles, C.byref(p))
        if not self._h:
            raise _lib.RmError(_lib.last_error())

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().rm_session_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def push(self, vehicle, time, lon, lat, accuracy=None, stamp_ms=0):
        """Append arrivals (in arrival order) and run every trigger they cause; returns the call's
        counts (SESSION_COUNTS).  stamp_ms: the stream time of each arrival, or one for all."""
        vehicle = _c(vehicle, np.uint32)
        n = len(vehicle)
        time = _c(time, np.float64)
        lon = _c(lon, np.float32)
        lat = _c(lat, np.float32)
        accuracy = None if accuracy is None else _c(accuracy, np.float32)
        stamp = _c(np.full(n, stamp_ms, np.int64) if np.ndim(stamp_ms) == 0 else stamp_ms, np.int64)
        if not (len(time) == len(lon) == len(lat) == len(stamp) == n) or (accuracy is not None and len(accuracy) != n):
            raise ValueError("arrival arrays must have equal lengths")
        d = _lib.RmSessionPoints(n, vehicle.ctypes.data, time.ctypes.data, lon.ctypes.data, lat.ctypes.data,
                                 accuracy.ctypes.data if accuracy is not None else None, stamp.ctypes.data)
        out = (C.c_uint64 * 8)()
        _lib.check(_lib.lib().rm_session_push(self._h, C.byref(d), out))
        return dict(zip(SESSION_COUNTS, (int(x) for x in out)))

    def push_messages(self, chunks, fmt, directory, stamp_ms=None, strict=False, shard=None):
        """Raw messages (one per line, in `chunks`) read, keyed through `directory` and pushed, all
        on the GPU (DESIGN.md §3 rule 14).  stamp_ms: the stream time of the whole call, or None
        for each message's own time.  Returns (push counts, line counts): SESSION_COUNTS and
        MESSAGES_INFO.  A tolerant call drops malformed messages (dropped_messages() lists them).
        shard=(rank, nranks): the masked push of a stream on several ranks (rule 16) -- everything is
        read and keyed, only the points of the vehicles `rank` owns are appended and matched; the
        line counts then carry "own" and "foreign", the points of either kind."""
        d, keep = _messages_desc(chunks, fmt, strict, stamp_ms)
        out = (C.c_uint64 * 8)()
        info = (C.c_uint64 * 8)()
        h = getattr(directory, "_h", None)
        if shard is None:
            _lib.check(_lib.lib().rm_session_push_messages(self._h, h, C.byref(d), out, info))
            own = None
        else:
            rank, nranks = (int(x) for x in shard)
            own = (C.c_uint64 * 2)()
            _lib.check(_lib.lib().rm_session_push_messages_sharded(self._h, h, C.byref(d), nranks, rank, out, info, own))
        info = dict(zip(MESSAGES_INFO, (int(x) for x in info)))
        if own is not None:
            info["own"], info["foreign"] = int(own[0]), int(own[1])
        return dict(zip(SESSION_COUNTS, (int(x) for x in out))), info

    def dropped_messages(self):
        """The first (at most 64) messages the last push_messages dropped: (chunk, line, reason)."""
        nd = C.c_uint32(0)
        dchunk = (C.c_uint32 * 64)()
        dline = (C.c_uint64 * 96)()
        reasons = C.create_string_buffer(64 * 96)
        _lib.check(_lib.lib().rm_session_dropped_messages(self._h, C.byref(nd), C.addressof(dchunk), C.addressof(dline),
                                                          C.addressof(reasons), 64 * 96))
        return _dropped(nd, dchunk, dline, reasons)

    def messages_span(self):
        """(smallest, largest) time among the points the last push_messages kept, or None for none."""
        t = (C.c_double * 2)()
        n = C.c_uint64(0)
        _lib.check(_lib.lib().rm_session_messages_span(self._h, t, C.byref(n)))
        return (float(t[0]), float(t[1])) if n.value else None

    def messages_ms(self):
        """Device ms of the last push_messages: upload, parse, ids, directory, then ms()'s five."""
        t = (C.c_double * 9)()
        _lib.check(_lib.lib().rm_session_messages_time(self._h, t))
        return dict(zip(("text_upload", "parse", "ids", "directory", "upload", "append", "trigger", "match", "trim"),
                        (float(x) for x in t)))

    def punctuate(self, timestamp_ms):
        out = (C.c_uint64 * 8)()
        _lib.check(_lib.lib().rm_session_punctuate(self._h, int(timestamp_ms), out))
        return dict(zip(SESSION_COUNTS, (int(x) for x in out)))

    def reports(self):
        n = C.c_uint64(0)
        _lib.check(_lib.lib().rm_session_get_reports(self._h, None, C.byref(n)))
        a = np.empty(max(n.value, 1), SESSION_REPORT_DTYPE)
        _lib.check(_lib.lib().rm_session_get_reports(self._h, a.ctypes.data, C.byref(n)))
        return a[: n.value]

    def windows(self):
        n = C.c_uint64(0)
        _lib.check(_lib.lib().rm_session_get_windows(self._h, None, C.byref(n)))
        a = np.empty(max(n.value, 1), SESSION_WINDOW_DTYPE)
        _lib.check(_lib.lib().rm_session_get_windows(self._h, a.ctypes.data, C.byref(n)))
        return a[: n.value]

    def store(self):
        """Per vehicle cnt, max_sep, last_update and the kept points packed in vehicle order
        (vehicle v's are [off[v], off[v + 1]))."""
        V = self.n_vehicles
        cnt = np.zeros(V, np.uint32)
        sep = np.zeros(V, np.float32)
        upd = np.zeros(V, np.int64)
        n = C.c_uint64(0)
        _lib.check(_lib.lib().rm_session_get_store(self._h, cnt.ctypes.data, None, None, None, None, None, None, C.byref(n)))
        m = max(int(n.value), 1)
        lon, lat, acc = np.zeros(m, np.float32), np.zeros(m, np.float32), np.zeros(m, np.float32)
        time = np.zeros(m, np.float64)
        _lib.check(_lib.lib().rm_session_get_store(self._h, cnt.ctypes.data, sep.ctypes.data, upd.ctypes.data, lon.ctypes.data,
                                                   lat.ctypes.data, time.ctypes.data, acc.ctypes.data, C.byref(n)))
        k = int(n.value)
        off = np.zeros(V + 1, np.uint64)
        np.cumsum(cnt, out=off[1:])
        return {"cnt": cnt, "max_sep": sep, "last_update": upd, "off": off, "lon": lon[:k], "lat": lat[:k],
                "time": time[:k], "accuracy": acc[:k]}

    def ms(self):
        """Device ms of the last call: upload, append, trigger, match, trim."""
        t = (C.c_double * 5)()
        _lib.check(_lib.lib().rm_session_time(self._h, t))
        return dict(zip(("upload", "append", "trigger", "match", "trim"), (float(x) for x in t)))


TILE_SEGMENT_DTYPE = np.dtype([
    ("id", "<u8"), ("next_id", "<u8"), ("t0", "<f8"), ("t1", "<f8"), ("length", "<i4"), ("queue_length", "<i4")])
assert TILE_SEGMENT_DTYPE.itemsize == 40
TILE_ADD_COUNTS = ("kept", "skipped", "rows", "held")
TILE_FLUSH_COUNTS = ("rows_in", "rows_kept", "tiles", "files", "bytes")
TILE_EXCHANGE_COUNTS = ("before", "sent", "received", "held")


def vehicle_owner(index, nranks):
    """The rank that holds directory index `index`'s session in a stream of nranks ranks (rule 16)."""
    return int(_lib.lib().rm_vehicle_owner(int(index), int(nranks)))


def tile_file_owner(bucket, tile, nranks):
    """The rank that culls and writes the file of time bucket `bucket` and tile id `tile`."""
    return int(_lib.lib().rm_tile_file_owner(int(bucket), int(tile), int(nranks)))


class TileStore:
    """The streaming anonymiser of the reference (AnonymisingProcessor.java) kept on the GPU
    (rm_tilestore_*; DESIGN.md §3 rule 13).  add() / add_session() are process(): segment pairs
    drop into every time-quantised tile they touch; flush() is punctuate(): every tile sorted,
    culled by the privacy count and written as the datastore's CSV body, all on the device."""

    def __init__(self, device=0, quantisation=3600, privacy=2, source="smpl_rprt", mode="auto", initial_rows=1 << 16):
        enc = lambda x: x if isinstance(x, bytes) else str(x).encode()
        tp = _lib.RmTileParams(int(quantisation), int(privacy), enc(source), enc(mode))
        self._h = _lib.lib().rm_tilestore_create(int(device), C.byref(tp), int(initial_rows))
        if not self._h:
            raise _lib.RmError(_lib.last_error())

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().rm_tilestore_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def add(self, id, next_id, t0, t1, length, queue_length):
        """Segments as arrays, in arrival order; returns the call's counts (TILE_ADD_COUNTS)."""
        n = len(id)
        cols = (_c(id, np.uint64), _c(next_id, np.uint64), _c(t0, np.float64), _c(t1, np.float64), _c(length, np.int32),
                _c(queue_length, np.int32))
        if any(len(x) != n for x in cols):
            raise ValueError("segment arrays must have equal lengths")
        a = np.empty(max(n, 1), TILE_SEGMENT_DTYPE)
        for name, x in zip(TILE_SEGMENT_DTYPE.names, cols):
            a[name][:n] = x
        out = (C.c_uint64 * 4)()
        _lib.check(_lib.lib().rm_tilestore_add(self._h, a.ctypes.data, n, out))
        return dict(zip(TILE_ADD_COUNTS, (int(x) for x in out)))

    def add_session(self, vehicle_sessions):
        """The forwarded reports of the session's last push / punctuate, device to device."""
        out = (C.c_uint64 * 4)()
        _lib.check(_lib.lib().rm_tilestore_add_session(self._h, getattr(vehicle_sessions, "_h", None), out))
        return dict(zip(TILE_ADD_COUNTS, (int(x) for x in out)))

    def flush(self):
        """(files, counts): an ordered dict name -> body bytes and TILE_FLUSH_COUNTS; empties the store."""
        blob = C.c_void_p()
        n = C.c_size_t()
        out = (C.c_uint64 * 5)()
        _lib.check(_lib.lib().rm_tilestore_flush(self._h, C.byref(blob), C.byref(n), out))
        try:
            raw = C.string_at(blob.value, n.value) if n.value else b""
        finally:
            _lib.lib().rm_free(blob)
        parts = raw.split(b"\0")
        files = {parts[i].decode(): parts[i + 1] for i in range(0, len(parts) - 1, 2)}
        return files, dict(zip(TILE_FLUSH_COUNTS, (int(x) for x in out)))

    def export_rows(self):
        """The rows held and their keys as bytes (rm_tilestore_export_rows, rule 16); the store keeps them."""
        blob = C.c_void_p()
        n = C.c_size_t()
        _lib.check(_lib.lib().rm_tilestore_export_rows(self._h, C.byref(blob), C.byref(n)))
        try:
            return C.string_at(blob.value, n.value)
        finally:
            _lib.lib().rm_free(blob)

    def import_owned(self, blobs, rank, nranks):
        """Replace the store's contents by the rows of `blobs` (every rank's export_rows, in rank
        order) whose file `rank` owns, merged into the one-rank store's order; returns TILE_EXCHANGE_COUNTS."""
        blobs = [bytes(b) for b in blobs]
        n = len(blobs)
        ptrs = (C.c_char_p * max(n, 1))(*blobs)
        lens = (C.c_size_t * max(n, 1))(*[len(b) for b in blobs])
        out = (C.c_uint64 * 4)()
        _lib.check(_lib.lib().rm_tilestore_import_owned(self._h, C.cast(ptrs, C.c_void_p), C.cast(lens, C.c_void_p), n,
                                                        int(nranks), int(rank), out))
        return dict(zip(TILE_EXCHANGE_COUNTS, (int(x) for x in out)))

    def exchange(self, comm):
        """export -> all-gather -> import on the device through a dist.Comm (rule 16): every rank
        calls it just before flush(); returns TILE_EXCHANGE_COUNTS."""
        out = (C.c_uint64 * 4)()
        _lib.check(_lib.lib().rm_tilestore_exchange(self._h, getattr(comm, "_h", None), out))
        return dict(zip(TILE_EXCHANGE_COUNTS, (int(x) for x in out)))

    def exchange_ms(self):
        """Device ms of the last import_owned / exchange: partition, transport, merge."""
        t = (C.c_double * 3)()
        _lib.check(_lib.lib().rm_tilestore_exchange_time(self._h, t))
        return dict(zip(("partition", "transport", "merge"), (float(x) for x in t)))

    def ms(self):
        """Device ms of the last call: upload, expand, sort, cull, text, download."""
        t = (C.c_double * 6)()
        _lib.check(_lib.lib().rm_tilestore_time(self._h, t))
        return dict(zip(("upload", "expand", "sort", "cull", "text", "download"), (float(x) for x in t)))


SNAPSHOT_COUNTS = ("bytes", "names", "vehicles", "points", "rows", "user_bytes")
SNAPSHOT_INFO = ("version", "bytes", "names", "vehicles", "points", "rows", "quantisation", "user_offset", "user_bytes")


def _snapshot_handle(obj, what):
    """None stays None (the section is left out or skipped); a closed object raises."""
    if obj is None:
        return None
    if not getattr(obj, "_h", None):
        raise _lib.RmError("%s is closed" % what)
    return obj._h


def save_stream(sessions=None, directory=None, store=None, user=b""):
    """The state of a stream as one blob (rm_snapshot_save; DESIGN.md §3 rule 15): the sessions' open
    point lists, the directory's names and the tile store's rows, any of them left out when None,
    with `user` bytes carried opaque.  Changes nothing the stream will output."""
    blob = C.c_void_p()
    n = C.c_size_t()
    out = (C.c_uint64 * 6)()
    ms = (C.c_double * 6)()
    user = bytes(user)
    handles = (_snapshot_handle(sessions, "sessions"), _snapshot_handle(directory, "directory"), _snapshot_handle(store, "store"))
    _lib.check(_lib.lib().rm_snapshot_save(*handles, user, len(user), C.byref(blob), C.byref(n), out, ms))
    try:
        raw = C.string_at(blob.value, n.value)
    finally:
        _lib.lib().rm_free(blob)
    save_stream.last = dict(zip(SNAPSHOT_COUNTS, (int(x) for x in out)),
                            ms=dict(zip(("pack", "gather", "checksum", "download"), (float(x) for x in ms))))
    return raw


def load_stream(blob, sessions=None, directory=None, store=None):
    """Restore save_stream's blob into empty objects (rm_snapshot_load); a None object's section is
    skipped.  Returns the counts (SNAPSHOT_COUNTS) and the device ms of upload, check and unpack.  A
    load that raises leaves the objects empty and usable."""
    blob = bytes(blob)
    out = (C.c_uint64 * 6)()
    ms = (C.c_double * 6)()
    handles = (_snapshot_handle(sessions, "sessions"), _snapshot_handle(directory, "directory"), _snapshot_handle(store, "store"))
    _lib.check(_lib.lib().rm_snapshot_load(*handles, blob, len(blob), out, ms))
    return dict(zip(SNAPSHOT_COUNTS, (int(x) for x in out)),
                ms=dict(zip(("upload", "check", "unpack"), (float(x) for x in ms))))


def snapshot_info(blob):
    """Check a snapshot on the host alone (rm_snapshot_check_host_shard: header, table, checksums and
    the structural rule) and return its numbers (SNAPSHOT_INFO) and its user bytes; a sharded
    stream's blob (rule 17) also gives rank, nranks and calls.  Raises with the reason."""
    blob = bytes(blob)
    info = (C.c_uint64 * 12)()
    err = C.create_string_buffer(512)
    if _lib.lib().rm_snapshot_check_host_shard(blob, len(blob), info, err, 512) != 0:
        raise _lib.RmError(err.value.decode("utf-8", "replace"))
    d = dict(zip(SNAPSHOT_INFO, (int(x) for x in info)))
    d["user"] = blob[d["user_offset"]:d["user_offset"] + d["user_bytes"]]
    if info[10]:
        d.update(rank=int(info[9]), nranks=int(info[10]), calls=int(info[11]))
    return d


def save_stream_shard(sessions=None, directory=None, store=None, shard=(0, 1), user=b""):
    """Rank shard[0]'s blob of a stream of shard[1] ranks (rm_snapshot_save_shard; DESIGN.md §3 rule
    17): save_stream's sections, the tile rows' keys and the shard record.  The store is needed and
    keeps keys from here on; nothing the stream will output changes."""
    blob = C.c_void_p()
    n = C.c_size_t()
    out = (C.c_uint64 * 6)()
    ms = (C.c_double * 6)()
    user = bytes(user)
    rank, nranks = (int(x) for x in shard)
    handles = (_snapshot_handle(sessions, "sessions"), _snapshot_handle(directory, "directory"), _snapshot_handle(store, "store"))
    _lib.check(_lib.lib().rm_snapshot_save_shard(*handles, rank, nranks, user, len(user), C.byref(blob), C.byref(n), out, ms))
    try:
        raw = C.string_at(blob.value, n.value)
    finally:
        _lib.lib().rm_free(blob)
    save_stream_shard.last = dict(zip(SNAPSHOT_COUNTS, (int(x) for x in out)),
                                  ms=dict(zip(("pack", "gather", "checksum", "download"), (float(x) for x in ms))))
    return raw


SNAPSHOT_SHARD_COUNTS = SNAPSHOT_COUNTS + ("calls", "saved_ranks")


def load_stream_shards(blobs, sessions=None, directory=None, store=None, shard=(0, 1)):
    """Restore, into empty objects, what rank shard[0] of shard[1] holds of the state that the blobs'
    ranks saved (rm_snapshot_load_shards): `blobs` are all the blobs of one save_stream_shard round in
    any order, or one save_stream blob, which counts as rank 0 of 1.  Returns the counts
    (SNAPSHOT_SHARD_COUNTS) and the device ms of upload, check, unpack and the rows' merge.  A load
    that raises leaves the objects empty and usable."""
    blobs = [bytes(b) for b in blobs]
    n = len(blobs)
    ptrs = (C.c_char_p * max(n, 1))(*blobs)
    lens = (C.c_size_t * max(n, 1))(*[len(b) for b in blobs])
    out = (C.c_uint64 * 8)()
    ms = (C.c_double * 6)()
    rank, nranks = (int(x) for x in shard)
    handles = (_snapshot_handle(sessions, "sessions"), _snapshot_handle(directory, "directory"), _snapshot_handle(store, "store"))
    _lib.check(_lib.lib().rm_snapshot_load_shards(*handles, C.cast(ptrs, C.c_void_p), C.cast(lens, C.c_void_p), n, rank, nranks,
                                                  out, ms))
    return dict(zip(SNAPSHOT_SHARD_COUNTS, (int(x) for x in out)),
                ms=dict(zip(("upload", "check", "unpack", "rows"), (float(x) for x in ms))))


def split_by_points(trace_off, parts):
    """Trace index cuts [0, ..., T] of `parts` contiguous ranges with about equal point counts
    (a cut where the running point count crosses k * P / parts); empty ranges are dropped."""
    trace_off = np.asarray(trace_off, np.uint64)
    T = len(trace_off) - 1
    P = int(trace_off[-1]) if T >= 0 else 0
    cuts = [0] + [int(np.searchsorted(trace_off, P * k / parts)) for k in range(1, max(1, int(parts)))] + [T]
    return sorted(set(min(max(c, 0), T) for c in cuts))


class MultiMatcher:
    """One batch as `parts` contiguous trace ranges (balanced by points), each on its own
    BatchMatcher (HIP stream + workspace).  rerun() runs every part at once
    (rm_runners_rerun: one host thread per part), so one part's gather-latency-bound stages
    (K2 route probes, the path walk) overlap another part's issue-bound ones (K1, K3).  Every
    point of the batch is matched once per rerun; a shared histogram is zeroed once."""

    def __init__(self, engine, parts=2):
        self.engine = engine
        self.parts = max(1, int(parts))
        self.bms = []

    def run(self, trace_off, lon, lat, time, accuracy=None, opts=None, trace_opt=None, **rp_kw):
        trace_off = np.asarray(trace_off, np.uint64)
        T = len(trace_off) - 1
        P = int(trace_off[-1])
        accuracy = np.full(P, -1.0, np.float32) if accuracy is None else np.asarray(accuracy, np.float32)
        trace_opt = np.zeros(T, np.uint32) if trace_opt is None else np.asarray(trace_opt, np.uint32)
        cuts = split_by_points(trace_off, self.parts)
        for bm in self.bms:
            bm.close()
        self.bms = []
        zero = rp_kw.pop("zero_hist", False)
        if zero and rp_kw.get("hist_dev"):
            _lib.check(_lib.lib().rm_device_memset(rp_kw["hist_dev"], 0, self.engine.n_segments * 16 * 4))
        if zero and rp_kw.get("dur_dev"):
            _lib.check(_lib.lib().rm_device_memset(rp_kw["dur_dev"], 0, self.engine.n_segments * 8))
        for t0, t1 in zip(cuts[:-1], cuts[1:]):
            if t1 <= t0:
                continue
            o0, o1 = int(trace_off[t0]), int(trace_off[t1])
            bm = BatchMatcher(self.engine)
            bm.run(trace_off[t0:t1 + 1] - o0, lon[o0:o1], lat[o0:o1], time[o0:o1], accuracy[o0:o1], opts,
                   trace_opt[t0:t1], **rp_kw)
            self.bms.append(bm)
        return self

    def rerun(self, **rp_kw):
        rp = BatchMatcher.run_params(**rp_kw)
        hs = (C.c_void_p * len(self.bms))(*[bm._h for bm in self.bms])
        _lib.check(_lib.lib().rm_runners_rerun(hs, len(self.bms), C.byref(rp)))

    def set_timing(self, on=True):
        for bm in self.bms:
            bm.set_timing(on)

    def set_timing_stages(self, names):
        for bm in self.bms:
            bm.set_timing_stages(names)

    def reset_times(self):
        for bm in self.bms:
            bm.reset_times()

    def kernel_times(self):
        """Per stage: (ms summed over the parts' launches, launches) — each launch timed by HIP
        events on its own stream while the other parts run."""
        out = {}
        for bm in self.bms:
            for k, (ms, n) in bm.kernel_times().items():
                a, b = out.get(k, (0.0, 0))
                out[k] = (a + ms, b + n)
        return out

    def sizes(self):
        out = {}
        for bm in self.bms:
            for k, v in bm.sizes().items():
                out[k] = out.get(k, 0) + v
        return out

    def set_locality(self, mode):
        for bm in self.bms:
            bm.set_locality(mode)

    def locality_used(self):
        return any(bm.locality_used() for bm in self.bms)

    def route_tiers(self):
        out = {}
        for bm in self.bms:
            for k, v in bm.route_tiers().items():
                out[k] = out.get(k, 0) + v
        return out

    def close(self):
        for bm in self.bms:
            bm.close()
        self.bms = []


def report_segments(seg_off, segs, trace_end_time, threshold_sec, report_mask, transition_mask):
    """The device report() epilogue (rm_report_segments) over host segment lists.
    seg_off: n+1 offsets into segs (SEGMENT_DTYPE); per-trace end time, threshold and level
    masks (scalars broadcast).  Returns (rep_off, reports REPORT_DTYPE, stats STATS_DTYPE)."""
    seg_off = _c(seg_off, np.uint32)
    n = len(seg_off) - 1
    segs = np.ascontiguousarray(segs, SEGMENT_DTYPE)
    bc = lambda x, dt: _c(np.broadcast_to(np.asarray(x, dt), (n,)), dt)
    end, thr = bc(trace_end_time, np.float64), bc(threshold_sec, np.float64)
    rm, tm = bc(report_mask, np.uint32), bc(transition_mask, np.uint32)
    d = _lib.RmReportDesc(n, seg_off.ctypes.data, segs.ctypes.data if len(segs) else None, end.ctypes.data,
                          thr.ctypes.data, rm.ctypes.data, tm.ctypes.data)
    rep_off = np.zeros(n + 1, np.uint32)
    reps = np.empty(max(int(seg_off[-1]) if n else 0, 1), REPORT_DTYPE)
    stats = np.empty(max(n, 1), STATS_DTYPE)
    _lib.check(_lib.lib().rm_report_segments(C.byref(d), rep_off.ctypes.data, reps.ctypes.data, stats.ctypes.data))
    return rep_off, reps[: rep_off[-1]], stats[:n]


def _take_replies(buf, off):
    """The n replies (bytes) of a library-allocated packed buffer, which is released."""
    try:
        n = len(off) - 1
        blob = C.string_at(buf.value, int(off[n])) if n else b""
    finally:
        _lib.lib().rm_free(buf)
    return [blob[int(off[i]):int(off[i + 1])] for i in range(n)]


def report_replies(seg_off, segs, trace_end_time, threshold_sec, report_mask, transition_mask, writer=0):
    """report() and the complete /report reply of every trace (rm_report_replies, DESIGN.md rule 19)
    over host segment lists, arguments as report_segments.  writer 0: by size, 1: the host formats
    the downloaded records, 2: the text is written on the device.  Returns (replies, info) with info
    = dict(bytes, flagged, writer, device_ms)."""
    seg_off = _c(seg_off, np.uint32)
    n = len(seg_off) - 1
    segs = np.ascontiguousarray(segs, SEGMENT_DTYPE)
    bc = lambda x, dt: _c(np.broadcast_to(np.asarray(x, dt), (n,)), dt)
    end, thr = bc(trace_end_time, np.float64), bc(threshold_sec, np.float64)
    rm, tm = bc(report_mask, np.uint32), bc(transition_mask, np.uint32)
    d = _lib.RmReportDesc(n, seg_off.ctypes.data, segs.ctypes.data if len(segs) else None, end.ctypes.data,
                          thr.ctypes.data, rm.ctypes.data, tm.ctypes.data)
    buf = C.c_void_p()
    off = np.zeros(n + 1, np.uint64)
    info = np.zeros(4, np.uint64)
    _lib.check(_lib.lib().rm_report_replies(C.byref(d), int(writer), C.byref(buf), off.ctypes.data, info.ctypes.data))
    return _take_replies(buf, off), dict(bytes=int(info[0]), flagged=int(info[1]), writer=int(info[2]),
                                         device_ms=int(info[3]) / 1000.0)


def format_replies_host(seg_off, segs, rep_off, reps, stats):
    """The /report replies of given segment, report and stats records (rm_report_format_host): the
    formatting alone, no GPU."""
    seg_off, rep_off = _c(seg_off, np.uint32), _c(rep_off, np.uint32)
    n = len(seg_off) - 1
    segs = np.ascontiguousarray(segs, SEGMENT_DTYPE)
    reps = np.ascontiguousarray(reps, REPORT_DTYPE)
    stats = np.ascontiguousarray(stats, STATS_DTYPE)
    buf = C.c_void_p()
    off = np.zeros(n + 1, np.uint64)
    _lib.check(_lib.lib().rm_report_format_host(n, seg_off.ctypes.data, segs.ctypes.data if len(segs) else None,
                                                rep_off.ctypes.data, reps.ctypes.data if len(reps) else None,
                                                stats.ctypes.data if n else None, C.byref(buf), off.ctypes.data))
    return _take_replies(buf, off)


def segment_dicts(segs):
    """Match-reply segments (README.md:288-301 schema) from SEGMENT_DTYPE records."""
    out = []
    for r in segs:
        d = {}
        if int(r["flags"]) & 2:
            d["segment_id"] = int(r["segment_id"])
        ways = [int(r["way_first"])]
        if int(r["way_last"]) != int(r["way_first"]):
            ways.append(int(r["way_last"]))
        d["way_ids"] = ways
        d["start_time"] = float(r["start_time"]) if r["start_time"] != -1 else -1
        d["end_time"] = float(r["end_time"]) if r["end_time"] != -1 else -1
        d["queue_length"] = int(r["queue_length"])
        d["length"] = int(r["length"])
        d["internal"] = bool(int(r["flags"]) & 1)
        d["begin_shape_index"] = int(r["begin_shape_index"])
        d["end_shape_index"] = int(r["end_shape_index"])
        out.append(d)
    return out
