"""Checkpoints of the stream on several ranks restated (DESIGN.md §3 rule 17) over the sharded
model of tests/stream_shard_ref.py: the state of M ranks stopped behind a poll (save), and that
state dealt out to N ranks (reshard) -- a vehicle's open session to vehicle_owner(vehicle, N), a tile
row to tile_file_owner(its file, N), the rows of all saved ranks in rank order merged by one stable
sort on the key.  Plain Python over the models alone; nothing here touches the library.

Also the numpy writer for blobs with the two sections the rule adds (kinds 11 and 12), beside
tests/snapshot_ref.py's, for the tests that forge such blobs."""
import copy
import functools
import math
import struct

import numpy as np

import snapshot_ref as sn
import stream_shard_ref as ss

TILE_KEYS, SHARD_REC = 11, 12
ELEM = {**sn.ELEM, TILE_KEYS: 8, SHARD_REC: 16}
SHARD_DTYPE = np.dtype([("rank", "<u4"), ("nranks", "<u4"), ("calls", "<u4"), ("pad", "<u4")])
# TileStoreRow (tile_text.hpp), 64 bytes
ROW_DTYPE = np.dtype([("id", "<u8"), ("next_id", "<u8"), ("start", "<i8"), ("end", "<i8"), ("duration", "<i4"), ("length", "<i4"),
                      ("queue", "<i4"), ("tile", "<u4"), ("bucket", "<u8"), ("arrival", "<u8")])
assert ROW_DTYPE.itemsize == 64


def write(sections, counts=None):
    """tests/snapshot_ref.py write() with the element sizes of kinds 11 and 12."""
    n = len(sections)
    at = sn.align16(32 + 40 * n)
    table, body = [], b""
    for kind, data in sections.items():
        data = bytes(data)
        count = (counts or {}).get(kind, len(data) // ELEM[kind])
        table.append((kind, ELEM[kind], at, len(data), count, sn.checksum(data)))
        body += data + b"\0" * (-len(data) % 16)
        at += sn.align16(len(data))
    ents = b"".join(struct.pack(sn.ENTRY, *e) for e in table)
    tsum = sn.checksum(struct.pack(sn.HEADER, sn.MAGIC, sn.VERSION, n, at, 0) + ents)
    head = struct.pack(sn.HEADER, sn.MAGIC, sn.VERSION, n, at, tsum) + ents
    return head + b"\0" * (-len(head) % 16) + body


# ---------------- the model ----------------
def drive_from(model, sc, stop):
    """The rest of the scenario behind `stop` polls."""
    out = []
    for k, (a, b) in enumerate(sc["polls"]):
        if k < stop:
            continue
        model.push(sc["pts"], a, b)
        if k in sc["flush_after"]:
            out.append(model.flush())
    model.punctuate(sc["ts"])
    out.append(model.flush())
    return out


def save(m):
    """What each rank of the sharded model m saves: its non-empty sessions by vehicle, its rows as
    (key, file, Seg) in store order, and the record."""
    out = []
    for rk in m.ranks:
        recs = [(v, copy.deepcopy(b)) for v, b in enumerate(rk.sessions.v) if len(b)]
        out.append({"rank": rk.rank, "nranks": m.nranks, "calls": m.calls, "records": recs, "rows": list(rk.rows)})
    return out


def as_plain(saved):
    """A one-rank save as rm_snapshot_save writes it and rule 17 reads it: no keys, so the rows are
    keyed by their position under call 0, and the next call is 1."""
    (b,) = saved
    rows = [(k, file, seg) for k, (_, file, seg) in enumerate(b["rows"])]
    return [dict(b, rows=rows, calls=1)]


def reshard(saved, N, sc):
    """The saved state dealt out to a fresh sharded model of N ranks."""
    M = len(saved)
    assert sorted(b["rank"] for b in saved) == list(range(M)) and all(b["nranks"] == M for b in saved)
    assert len(set(b["calls"] for b in saved)) == 1
    m = ss.ShardedStream(N, sc["n_vehicles"], sc["match_fn"], ss.PARAMS, ss.Q, ss.PRIVACY)
    m.calls = saved[0]["calls"]
    seen = set()
    for b in saved:
        for v, veh in b["records"]:
            assert v not in seen, "a vehicle in two blobs"
            seen.add(v)
            m.ranks[ss.vehicle_owner(v, N)].sessions.v[v] = copy.deepcopy(veh)
    gathered = [row for b in sorted(saved, key=lambda b: b["rank"]) for row in b["rows"]]
    for rk in m.ranks:
        mine = [row for row in gathered if ss.tile_file_owner(row[1][0] // ss.Q, row[1][1], N) == rk.rank]
        rk.rows = sorted(mine, key=lambda row: row[0])   # stable
    return m


def row_tuple(key, file, seg):
    return (int(key), file[0] // ss.Q, file[1], seg.id, seg.next_id, math.floor(seg.min), math.ceil(seg.max), seg.length, seg.queue)


def rank_state(rk):
    """What a save of this rank must hold, in comparable form: records as (vehicle, cnt, max_sep bits,
    last_update, lon, lat, acc, time bytes) and rows as (key, bucket, tile, id, next_id, start, end,
    length, queue) in store order."""
    F = np.float32
    recs = [(v, len(b), F(b.max_sep).tobytes(), int(b.last_update), np.array(b.lon, F).tobytes(), np.array(b.lat, F).tobytes(),
             np.array(b.acc, F).tobytes(), np.array(b.time, np.float64).tobytes())
            for v, b in enumerate(rk.sessions.v) if len(b)]
    return recs, [row_tuple(*row) for row in rk.rows]


def blob_state(blob):
    """The same from a library blob (sections by tests/snapshot_ref.py read())."""
    secs, _ = sn.read(blob)
    rec = np.frombuffer(secs[sn.SESS_REC], sn.REC_DTYPE)
    lon, lat, acc = (np.frombuffer(secs[k], "<f4") for k in (sn.SESS_LON, sn.SESS_LAT, sn.SESS_ACC))
    time = np.frombuffer(secs[sn.SESS_TIME], "<f8")
    recs, at = [], 0
    for r in rec:
        c = int(r["cnt"])
        recs.append((int(r["vehicle"]), c, np.float32(r["max_sep"]).tobytes(), int(r["last_update"]), lon[at:at + c].tobytes(),
                     lat[at:at + c].tobytes(), acc[at:at + c].tobytes(), time[at:at + c].tobytes()))
        at += c
    row = np.frombuffer(secs[sn.TILE_ROWS], ROW_DTYPE)
    keys = np.frombuffer(secs[TILE_KEYS], "<u8") if TILE_KEYS in secs else np.arange(len(row), dtype="<u8")
    return recs, [(int(k), int(r["bucket"]), int(r["tile"]), int(r["id"]), int(r["next_id"]), int(r["start"]), int(r["end"]),
                   int(r["length"]), int(r["queue"])) for k, r in zip(keys, row)]


def cases(saved, N, before_next_flush):
    """What a save of M ranks at one stop and its reshard to N show of the cases rule 17's tests need.
    before_next_flush: the resharded model's rows per rank before the exchange of its first later flush."""
    M = len(saved)
    out = {"every_rank_has_sessions": all(len(b["records"]) > 0 for b in saved),
           "a_rank_has_rows": any(len(b["rows"]) > 0 for b in saved),
           "vehicle_changes_owner": sum(1 for b in saved for v, _ in b["records"] if ss.vehicle_owner(v, N) != b["rank"]),
           "row_changes_holder": sum(1 for b in saved for _, file, _ in b["rows"]
                                     if ss.tile_file_owner(file[0] // ss.Q, file[1], N) != b["rank"])}
    # a run of the next flush with saved rows of two blobs that meets the privacy count only with both
    src = {id(seg): b["rank"] for b in saved for _, _, seg in b["rows"]}
    runs = {}
    for rows in before_next_flush:
        for _, file, seg in rows:
            if id(seg) in src:
                runs.setdefault((file, seg.id, seg.next_id), [0] * M)[src[id(seg)]] += 1
    out["file_needs_two_blobs"] = sum(1 for c in runs.values() if sum(c) >= ss.PRIVACY and max(c) < ss.PRIVACY)
    return out


@functools.lru_cache(maxsize=4)
def stops(path, M):
    """The M-rank model stopped behind 1, 2, ... polls: per stop (the flushes' files so far, the saved state)."""
    sc = ss.scenario(path)
    m = ss.ShardedStream(M, sc["n_vehicles"], sc["match_fn"], ss.PARAMS, ss.Q, ss.PRIVACY)
    out, flushes = [], []
    for k, (a, b) in enumerate(sc["polls"]):
        m.push(sc["pts"], a, b)
        if k in sc["flush_after"]:
            flushes.append(m.flush())
        saved = save(m)
        out.append((list(flushes), as_plain(saved) if M == 1 else saved))
    return out


@functools.lru_cache(maxsize=64)
def resume(path, M, N, stop):
    """Stop the M-rank model behind `stop` polls, reshard to N, continue.  before: the files of the
    flushes before the stop; saved; loaded: rank_state per rank as loaded; files: the later flushes'
    files per rank; cases."""
    sc = ss.scenario(path)
    before, saved = stops(path, M)[stop - 1]
    m = reshard(saved, N, sc)
    loaded = [rank_state(rk) for rk in m.ranks]
    files = drive_from(m, sc, stop)
    return {"before": before, "saved": saved, "loaded": loaded, "files": files, "cases": cases(saved, N, m.before[0]), "model": m}


PAIRS = [(M, N) for M in (1, 2, 3) for N in (1, 2, 3) if M != N]


def shows_every_case(c, M):
    """(a file that needs two blobs wants M >= 2: one saved rank writes one blob)"""
    return bool(c["every_rank_has_sessions"] and c["a_rank_has_rows"] and c["vehicle_changes_owner"] > 0
                and c["row_changes_holder"] > 0 and (M == 1 or c["file_needs_two_blobs"] > 0))


@functools.lru_cache(maxsize=2)
def choose_stop(path):
    """The first stop position (polls made) at which every (M, N) in PAIRS shows every case."""
    sc = ss.scenario(path)
    for stop in range(1, len(sc["polls"]) + 1):
        if all(shows_every_case(resume(path, M, N, stop)["cases"], M) for M, N in PAIRS):
            return stop
    raise AssertionError("no stop position shows every case")


def union(per_rank):
    """One flush's files of all ranks; each file from one rank."""
    out = {}
    for files in per_rank:
        assert not set(files) & set(out)
        out.update(files)
    return out
