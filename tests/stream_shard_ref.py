"""The stream on several ranks restated (DESIGN.md §3 rule 16) over the two sequential models: the
sessions of tests/stream_ref.py per rank over the vehicles it owns, every tile row keyed by
(add call, triggering arrival), the rows exchanged to the owners of their files and merged by one
stable sort on the key, then the anonymiser of tests/anonymiser_ref.py per rank.  The GPU form must
give, file for file, what the one-rank models give -- and so must this model, which the CPU test
checks first (with and, to keep the input honest, without the exchange).

Also the one small stream the rule's tests share (scenario): clone pairs of vehicles on conftest's
small_world, cut into five polls with two flushes in between and the final punctuate behind.
"""
import functools

import numpy as np

import anonymiser_ref as ar
import stream_ref as sr

MASK32, MASK64 = (1 << 32) - 1, (1 << 64) - 1


def vehicle_owner(index, nranks):
    """rm_common.hpp vehicle_owner: a Fibonacci hash of the index scaled to the rank count."""
    return (((index * 0x9E3779B1) & MASK32) * max(nranks, 1)) >> 32


def tile_file_owner(bucket, tile, nranks):
    """rm_common.hpp tile_file_owner."""
    h = ((((bucket << 25) & MASK64) | tile) * 0x9E3779B97F4A7C15) & MASK64
    return (h >> 33) % max(nranks, 1)


def seg_of(r):
    return (int(r["id"]), int(r["next_id"]), float(r["t0"]), float(r["t1"]), int(r["length"]), int(r["queue_length"]))


class Rank:
    """One rank: its sessions (every vehicle has a slot, only the owned ones ever hold points) and
    its tile rows in store order as (key, (start, tile id), Seg)."""

    def __init__(self, rank, nranks, n_vehicles, match_fn, params, q):
        self.rank, self.nranks, self.q = rank, nranks, q
        self.sessions = sr.Sessions(n_vehicles, match_fn, **params)
        self.rows = []
        self.n_rep = 0
        self.own = 0
        self.win_call = []   # per window of the sessions: the call that made it

    def add_reports(self, call):
        """rm_tilestore_add_session of the call just made: the new reports in the order the session
        gives them, each row keyed by its report's triggering arrival."""
        m = self.sessions
        self.win_call += [call] * (len(m.windows) - len(self.win_call))
        for r, _, w in m.reports[self.n_rep:]:
            seg = ar.Seg(*seg_of(r))
            assert ar.Anonymiser.limit(seg, self.q) is None and seg.valid()
            key = (call << 32) | m.windows[w][1]
            self.rows += [(key, file, seg) for file in ar.tiles_of(seg, self.q)]
        self.n_rep = len(m.reports)


class ShardedStream:
    """R ranks in lockstep.  push() takes a whole call's arrivals (every rank sees them all and
    appends the owned ones, tagged by their index in the call); flush() exchanges unless told not to."""

    def __init__(self, nranks, n_vehicles, match_fn, params, q, privacy):
        self.ranks = [Rank(r, nranks, n_vehicles, match_fn, params, q) for r in range(nranks)]
        self.nranks, self.q, self.privacy = nranks, q, privacy
        self.calls = 0
        self.exchanges = []   # per exchange and rank: rows before, sent away, received, held
        self.before = []      # per flush and rank: the rows it held before the exchange
        self.punctuate_call = None

    def push(self, p, a, b):
        for rk in self.ranks:
            for j in range(a, b):
                v = int(p["vehicle"][j])
                if vehicle_owner(v, self.nranks) != rk.rank:
                    continue
                rk.own += 1
                rk.sessions.arrive(v, p["time"][j], p["lon"][j], p["lat"][j], p["accuracy"][j], p["stamp_ms"][j], j - a)
            rk.add_reports(self.calls)
        self.calls += 1

    def punctuate(self, ts):
        self.punctuate_call = self.calls
        for rk in self.ranks:
            rk.sessions.punctuate(ts)
            rk.add_reports(self.calls)
        self.calls += 1

    def flush(self, exchange=True):
        """Per rank the files of anonymiser_ref's flush over the rows it holds then."""
        self.before.append([list(rk.rows) for rk in self.ranks])
        if exchange:
            gathered = [(row, rk.rank) for rk in self.ranks for row in rk.rows]   # ranks in rank order
            stats = []
            for rk in self.ranks:
                mine = [(row, src) for row, src in gathered
                        if tile_file_owner(row[1][0] // self.q, row[1][1], self.nranks) == rk.rank]
                kept_own = sum(1 for _, src in mine if src == rk.rank)
                stats.append({"before": len(rk.rows), "sent": len(rk.rows) - kept_own, "received": len(mine) - kept_own,
                              "held": len(mine)})
                rk.rows = sorted((row for row, _ in mine), key=lambda row: row[0])   # stable
            self.exchanges.append(stats)
        out = []
        for rk in self.ranks:
            anon = ar.Anonymiser(self.q, self.privacy)
            for _, file, seg in rk.rows:
                anon.tiles.setdefault(file, []).append(seg)
            out.append(anon.flush()[0])
            rk.rows = []
        return out


class OneRank:
    """The yardstick's model: stream_ref and anonymiser_ref as tests/test_gpu_stream.py joins them."""

    def __init__(self, n_vehicles, match_fn, params, q, privacy):
        self.sessions = sr.Sessions(n_vehicles, match_fn, **params)
        self.anon = ar.Anonymiser(q, privacy)
        self.n_rep = 0
        self.rows_at_flush = []

    def _add(self):
        self.anon.add([seg_of(r) for r, _, _ in self.sessions.reports[self.n_rep:]])
        self.n_rep = len(self.sessions.reports)

    def push(self, p, a, b):
        self.sessions.push(p["vehicle"][a:b], p["time"][a:b], p["lon"][a:b], p["lat"][a:b], p["accuracy"][a:b], p["stamp_ms"][a:b])
        self._add()

    def punctuate(self, ts):
        self.sessions.punctuate(ts)
        self._add()

    def flush(self):
        self.rows_at_flush.append(self.anon.held())
        return self.anon.flush()[0]


def drive(model, sc, **flush_kw):
    """The scenario's calls on a model: the flushes' results in order."""
    out = []
    for k, (a, b) in enumerate(sc["polls"]):
        model.push(sc["pts"], a, b)
        if k in sc["flush_after"]:
            out.append(model.flush(**flush_kw))
    model.punctuate(sc["ts"])
    out.append(model.flush(**flush_kw))
    return out


def cases(files, m):
    """What the sharded model, driven with the exchange, shows of the cases rule 16's tests must
    contain (files: per flush and rank, as drive gives them): each entry counts the occurrences."""
    R, q = m.nranks, m.q
    owner = lambda file: tile_file_owner(file[0] // q, file[1], R)
    out = dict.fromkeys(("run_needs_two_ranks", "double_trigger", "punctuate_rows", "segment_two_owners", "rank_without_file",
                         "rank_without_rows", "largest_exchange"), 0)
    for per_rank in m.before:
        runs = {}   # (file, id, next_id) -> rows per rank
        for r, rows in enumerate(per_rank):
            for _, file, seg in rows:
                runs.setdefault((file, seg.id, seg.next_id), [0] * R)[r] += 1
        out["run_needs_two_ranks"] += sum(1 for c in runs.values() if sum(c) >= m.privacy and max(c) < m.privacy)
        segs = {}   # a segment's files (one Seg object per report)
        for rows in per_rank:
            for _, file, seg in rows:
                segs.setdefault(id(seg), set()).add(owner(file))
        out["segment_two_owners"] += sum(1 for o in segs.values() if len(o) > 1)
        out["punctuate_rows"] += sum(1 for rows in per_rank for key, _, _ in rows if key >> 32 == m.punctuate_call)
        n = [len(rows) for rows in per_rank]
        out["rank_without_rows"] += sum(1 for x in n if x == 0 and max(n) > 0)
        out["largest_exchange"] = max(out["largest_exchange"], sum(n))
    for rk in m.ranks:
        seen = set()
        for w, call in zip(rk.sessions.windows, rk.win_call):
            out["double_trigger"] += (w[0], call) in seen and call != m.punctuate_call
            seen.add((w[0], call))
    for per_rank in files:
        if any(per_rank):
            out["rank_without_file"] += sum(1 for f in per_rank if not f)
    return out


# ---------------- the shared stream ----------------
PARAMS = dict(dist=800.0, count=8, time_s=60.0)
Q, PRIVACY = 60, 2
T0 = 1483228800 + 45          # (bucket boundaries fall 15 s into the stream and every 60 s from there)
RATE, N_PTS = 15.0, 40        # a point every 15 s; a cohort vehicle lives 600 s, the pair S three times that
N_PAIRS_A, N_PAIRS_B = 60, 59
CUTS = (0, 300, 600, 900, 1200, 1500, 1800)   # the polls in seconds of stream time
B_START = 1200         # cohort B starts this many seconds into the stream
FLUSH_AFTER = (1, 2)
BAD_EVERY = 397


def special_pair(lo, hi):
    """The first indices (k, k + 13) in [lo, hi) with one owner at 2 ranks and one at 3 (13 steps of
    the hash's golden-ratio stride land 0.034 of the range further on; neighbours never share both)."""
    for k in range(lo, hi - 13):
        if vehicle_owner(k, 2) == vehicle_owner(k + 13, 2) and vehicle_owner(k, 3) == vehicle_owner(k + 13, 3):
            return k, k + 13
    raise AssertionError("no pair of indices with one owner")


@functools.lru_cache(maxsize=2)
def scenario(path):
    """Cohort A: clone pairs living 600 s from T0; the special pair S: 1,800 s from T0, alone in the
    stream from 600 s to 1,200 s, its two vehicles with one owner at 2 and at 3 ranks; cohort B: clone
    pairs living 600 s from T0 + 1,200.  A pair's vehicles send identical points, so each run of a pair
    reaches the privacy count of 2 only with both.  Vehicles are numbered in first-seen order, which
    is the directory's."""
    from reporter_amd import engine, graphfile, world
    import msg_text
    n_first = 2 * N_PAIRS_A + 2                      # the vehicles seen at T0: cohort A and the pair S
    special = special_pair(20, n_first)
    free = [i for i in range(n_first) if i not in special]
    number = {"A": [free[2 * k:2 * k + 2] for k in range(N_PAIRS_A)], "S": [list(special)],
              "B": [[n_first + 2 * k, n_first + 2 * k + 1] for k in range(N_PAIRS_B)]}
    tr = {"A": world.generate_traces(path, N_PAIRS_A, N_PTS, rate_s=RATE, noise_m=5.0, seed=31, start_epoch=T0),
          "S": world.generate_traces(path, 1, 3 * N_PTS, rate_s=RATE, noise_m=5.0, seed=33, start_epoch=T0),
          "B": world.generate_traces(path, N_PAIRS_B, N_PTS, rate_s=RATE, noise_m=5.0, seed=32, start_epoch=T0 + int(B_START))}
    cols = {k: [] for k in ("vehicle", "time", "lon", "lat", "accuracy")}
    start = {"A": T0, "S": T0, "B": T0 + B_START}
    for part in ("A", "S", "B"):
        t = tr[part]
        off = t["trace_off"]
        for k in range(len(off) - 1):
            for v in number[part][k]:   # the clone pair
                n = int(off[k + 1] - off[k])
                cols["vehicle"].append(np.full(n, v, np.uint32))
                cols["time"].append(start[part] + RATE * np.arange(n, dtype=np.float64))   # (the generator staggers its starts)
                for name in ("lon", "lat", "accuracy"):
                    cols[name].append(np.asarray(t[name][off[k]:off[k + 1]]))
    n_vehicles = n_first + 2 * N_PAIRS_B
    cat = {k: np.concatenate(x) for k, x in cols.items()}
    order = np.lexsort((cat["vehicle"], cat["time"]))
    arr = {"vehicle": cat["vehicle"][order], "time": cat["time"].astype(np.float64)[order],
           "lon": cat["lon"].astype(np.float32)[order], "lat": cat["lat"].astype(np.float32)[order],
           "accuracy": cat["accuracy"].astype(np.float32)[order]}
    pts = msg_text.expected(arr)
    pts["stamp_ms"] = (pts["time"] * 1000.0).astype(np.int64)
    first_seen = arr["vehicle"][np.sort(np.unique(arr["vehicle"], return_index=True)[1])]
    assert first_seen.tolist() == list(range(n_vehicles))
    edges = np.searchsorted(arr["time"], [T0 + c for c in CUTS])
    polls = list(zip(edges[:-1].tolist(), edges[1:].tolist()))
    g = graphfile.load(path)
    return {"path": path, "arr": arr, "pts": pts, "polls": polls, "flush_after": FLUSH_AFTER, "n_vehicles": n_vehicles,
            "special": special, "ts": int(arr["time"].max() * 1000) + 10 ** 7,
            "match_fn": sr.oracle_matcher(g, engine.default_options(1)), "texts": [
                msg_text.text(arr, 0, a, b, bad_every=BAD_EVERY) for a, b in polls]}


@functools.lru_cache(maxsize=2)
def models(path):
    """The one-rank model's files per flush and, for 2 and 3 ranks, the sharded model driven with
    the exchange (its files per flush and rank, and the model itself for what the tests look up)."""
    sc = scenario(path)
    one = OneRank(sc["n_vehicles"], sc["match_fn"], PARAMS, Q, PRIVACY)
    out = {"one": drive(one, sc), "one_model": one}
    for R in (2, 3):
        m = ShardedStream(R, sc["n_vehicles"], sc["match_fn"], PARAMS, Q, PRIVACY)
        out[R] = (drive(m, sc), m)
    return out
