"""Vehicle sessions restated (DESIGN.md §3 rule 12): the reference's streaming batcher
(BatchingProcessor.java:57-141, Batch.java:35-90) as a sequential model in plain Python, one
arrival at a time, over the oracle's match() and report().  The GPU sessions (sessions.hip) must
give this model's windows, forwarded reports and final store bit for bit, however the arrivals
are cut into pushes.
"""
import math

import numpy as np

from matched_points_ref import det_cos

F = np.float32
MPD = 20037581.187 / 180.0          # Batch.java:36
RAD = math.pi / 180.0               # Batch.java:35
CAPPED = 0x80000000                 # window err: cleared at max_vehicle_points, not matched


def distance(alon, alat, blon, blat):
    """Batch.java:37-41 in Java's types: float difference and float mean, the rest double; cos is
    the project's det_cos (stated deviation from Math.cos)."""
    alon, alat, blon, blat = F(alon), F(alat), F(blon), F(blat)
    x = float(F(alon - blon)) * MPD * det_cos(float(F(F(0.5) * F(alat + blat))) * RAD)
    y = float(F(alat - blat)) * MPD
    return math.sqrt(x * x + y * y)


def fold(max_sep, d):
    """max_sep = (float)Math.max(max_sep, d) (Batch.java:45), as Java writes it."""
    return F(max(float(max_sep), d))


def fold_float(max_sep, d):
    """The same as a maximum of floats, the form a parallel prefix maximum takes."""
    f = F(d)
    return f if f > max_sep else F(max_sep)


def bails(max_sep, n, t0, tl, dist, count, time_s):
    return float(max_sep) < dist or n < count or tl - t0 < time_s   # Batch.java:51-53


def forwards(r):
    """Segment.valid() (Segment.java:38-40) on one report record."""
    return bool(r["t0"] > 0 and r["t1"] > 0 and r["t1"] > r["t0"] and r["length"] > 0 and r["queue_length"] >= 0)


def oracle_matcher(graph, opts, threshold_sec=15.0, report_mask=0x6, transition_mask=0x6):
    """match_fn over the oracle: one trace in, (error bits, shape_used or -1, reports) out."""
    import meili_oracle as mo

    def fn(vehicle, lon, lat, time, acc):
        n = len(lon)
        b = mo.Batch(np.array([0, n], np.uint32), lon, lat, time, acc, opts[:1], np.zeros(1, np.uint32))
        ref = mo.match(graph, b)
        segs = ref["segs"][ref["seg_off"][0]:ref["seg_off"][1]]
        reps, st = mo.report_trace(segs, time[-1], threshold_sec, report_mask, transition_mask)
        return 0, int(st["shape_used"]), reps

    return fn


class Vehicle:
    def __init__(self):
        self.lon, self.lat, self.time, self.acc = [], [], [], []
        self.max_sep = F(0)
        self.last_update = 0

    def __len__(self):
        return len(self.lon)

    def drop(self, k):
        del self.lon[:k], self.lat[:k], self.time[:k], self.acc[:k]


class Sessions:
    """The sequential model.  match_fn(vehicle, lon, lat, time, acc) -> (err, shape_used, reports)."""

    def __init__(self, n_vehicles, match_fn, dist=500.0, count=10, time_s=60.0, gap_ms=60000, max_points=0):
        self.v = [Vehicle() for _ in range(n_vehicles)]
        self.match_fn = match_fn
        self.dist, self.count, self.time_s, self.gap_ms, self.max_points = dist, count, time_s, gap_ms, max_points
        self.windows = []     # (vehicle, arrival tag, n_points, shape_used, n_reports, err) over all calls
        self.reports = []     # (report record, vehicle, index into windows)
        self.all_reports = []  # every report of every window, before the forwarding filter
        self.counts = dict(arrivals=0, triggers=0, trims=0, cleared=0, failed=0, forwarded=0, invalid=0)
        self.closest = float("inf")   # |evaluated distance - dist| at its smallest

    def _report(self, vi, tag, dist, count, time_s, evict=False):
        b = self.v[vi]
        n = len(b)
        if bails(b.max_sep, n, b.time[0], b.time[-1], dist, count, time_s):
            return False
        c = self.counts
        c["triggers"] += 1
        err, su, reps = self.match_fn(vi, np.array(b.lon, F), np.array(b.lat, F), np.array(b.time, np.float64),
                                      np.array(b.acc, F))
        w = len(self.windows)
        if err:
            c["failed"] += 1
            self.windows.append((vi, tag, n, -1, 0, err))
            b.drop(n)                       # the catch branch: Batch.java:83-87
            b.max_sep = F(0)
            return True
        self.windows.append((vi, tag, n, su, len(reps), 0))
        for r in reps:
            self.all_reports.append(r.copy())
            if forwards(r):
                self.reports.append((r.copy(), vi, w))
                c["forwarded"] += 1
            else:
                c["invalid"] += 1
        if su >= 0:
            c["trims"] += 1
            trim_to = min(su, n)
        else:
            c["cleared"] += 1
            trim_to = n                     # Batch.java:75
        b.drop(trim_to)
        b.max_sep = F(0)
        for i in range(1, len(b)):          # Batch.java:78-80
            b.max_sep = fold(b.max_sep, distance(b.lon[i], b.lat[i], b.lon[0], b.lat[0]))
        return True

    def arrive(self, vi, time, lon, lat, acc, stamp_ms, tag):
        """BatchingProcessor.process (:57-84); tag: the arrival's index in its push."""
        b = self.v[vi]
        if len(b) == 0:
            b.max_sep = F(0)
        else:
            d = distance(lon, lat, b.lon[0], b.lat[0])
            self.closest = min(self.closest, abs(d - self.dist))
            b.max_sep = fold(b.max_sep, d)
            self.counts["arrivals"] += 1
        b.lon.append(F(lon)); b.lat.append(F(lat)); b.time.append(float(time)); b.acc.append(F(acc))
        if len(b) > 1:
            fired = self._report(vi, tag, self.dist, self.count, self.time_s)
            if not fired and self.max_points > 0 and len(b) >= self.max_points:
                self.windows.append((vi, tag, len(b), -1, 0, CAPPED))
                b.drop(len(b))
                b.max_sep = F(0)
        if len(b) > 0:
            b.last_update = int(stamp_ms)
        else:
            b.last_update = 0

    def push(self, vehicle, time, lon, lat, acc=None, stamp_ms=0):
        n = len(vehicle)
        stamp = np.full(n, stamp_ms, np.int64) if np.ndim(stamp_ms) == 0 else stamp_ms
        for j in range(n):
            self.arrive(int(vehicle[j]), time[j], lon[j], lat[j], -1.0 if acc is None else acc[j], stamp[j], j)

    def punctuate(self, timestamp_ms):
        """:86-106, in vehicle-index order (stated deviation: the store iterates in key order)."""
        for vi, b in enumerate(self.v):
            if len(b) == 0 or not (timestamp_ms - b.last_update > self.gap_ms):
                continue
            self._report(vi, vi, 0.0, 2, 0.0, evict=True)
            b.drop(len(b))
            b.max_sep = F(0)
            b.last_update = 0

    def store(self):
        cnt = np.array([len(b) for b in self.v], np.uint32)
        cat = lambda name, dt: np.array([x for b in self.v for x in getattr(b, name)], dt)
        return {"cnt": cnt, "max_sep": np.array([b.max_sep for b in self.v], F),
                "last_update": np.array([b.last_update for b in self.v], np.int64),
                "lon": cat("lon", F), "lat": cat("lat", F), "time": cat("time", np.float64), "accuracy": cat("acc", F)}

    def window_array(self):
        from reporter_amd.engine import SESSION_WINDOW_DTYPE
        a = np.zeros(len(self.windows), SESSION_WINDOW_DTYPE)
        for k, w in enumerate(self.windows):
            a[k] = w
        return a

    def report_array(self):
        from reporter_amd.engine import SESSION_REPORT_DTYPE
        a = np.zeros(len(self.reports), SESSION_REPORT_DTYPE)
        for k, (r, vi, w) in enumerate(self.reports):
            for f in r.dtype.names:
                a[k][f] = r[f]
            a[k]["vehicle"], a[k]["window"] = vi, w
        return a

    def histogram(self, n_segments):
        """The speed histogram and duration sums a run accumulates (engine.hip k_report): over the
        successful reports -- all of them, forwarded or not -- that pass the tile rule."""
        hist = np.zeros(n_segments * 16, np.uint32)
        dur = np.zeros(n_segments, np.uint64)
        for r in self.all_reports:
            dt = float(r["t1"]) - float(r["t0"])
            if not (r["t0"] > 0 and r["t1"] > 0 and dt > 0.5 and r["length"] > 0 and r["queue_length"] >= 0):
                continue
            if int(r["seg_dense"]) == 0xFFFFFFFF:
                continue
            b = min(15, max(0, int((float(r["length"]) / dt) * 3.6 / 10.0)))
            hist[int(r["seg_dense"]) * 16 + b] += 1
            dur[int(r["seg_dense"])] += int(math.floor(dt + 0.5))
        return hist, dur


def interleave(tr, stamps_ms=None):
    """One trace per vehicle -> arrivals ordered by time, ties by vehicle: (vehicle, time, lon, lat,
    accuracy, stamp_ms) arrays.  stamps_ms: per arrival stream time (default: time in ms)."""
    off = tr["trace_off"]
    T = len(off) - 1
    veh = np.concatenate([np.full(int(off[k + 1] - off[k]), k, np.uint32) for k in range(T)])
    order = np.lexsort((veh, tr["time"]))
    out = {"vehicle": veh[order], "time": np.asarray(tr["time"], np.float64)[order],
           "lon": np.asarray(tr["lon"], F)[order], "lat": np.asarray(tr["lat"], F)[order],
           "accuracy": np.asarray(tr["accuracy"], F)[order]}
    out["stamp_ms"] = (out["time"] * 1000.0).astype(np.int64) if stamps_ms is None else np.asarray(stamps_ms, np.int64)[order]
    return out


def slices(arr, seconds):
    """Cut interleaved arrivals into pushes of `seconds` of data time (None: one push; 0: one
    point per vehicle per push, i.e. one push per distinct time)."""
    n = len(arr["vehicle"])
    if seconds is None:
        return [(0, n)]
    t = arr["time"]
    key = t if seconds == 0 else np.floor((t - t[0]) / seconds)
    cuts = [0] + [j for j in range(1, n) if key[j] != key[j - 1]] + [n]
    return list(zip(cuts[:-1], cuts[1:]))
