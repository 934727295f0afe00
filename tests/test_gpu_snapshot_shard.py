"""Checkpoints of the stream on several ranks on one GPU, in one process (DESIGN.md §3 rule 17): the
scenario of tests/stream_shard_ref.py runs on M ranks to the stop position the resharding model chose
(tests/snapshot_shard_ref.py; tests/test_snapshot_shard_ref.py asserts, from the models alone, that the
position shows every case), every rank saves its shard, everything is closed, N fresh sets of
objects load what they own of the M blobs and continue.  The yardstick is the one-rank stream that
never stopped, on the same polls: the union of the ranks' files of every later flush must be its
files byte for byte, the windows merged by arrival its windows, the names its names; and a save
straight after the load must hold, rank by rank, the model's resharded records and rows.

R sessions, directories and stores run on one engine, the exchange by export_rows / import_owned,
as tests/test_gpu_stream_shard.py does it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import snapshot_ref as sn
import snapshot_shard_ref as sh
import stream_shard_ref as ss
from reporter_amd import _lib, engine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(2, 2), (2, 3), (3, 2), (1, 2), (2, 1)]
FMT = lambda: engine.MessageFormat(0, engine.LineFormat())


class Ranks:
    """R sets of objects on one engine."""

    def __init__(self, eng, R, n_vehicles, sharded=True, rows0=8):
        self.R, self.sharded = R, sharded
        self.bms = [engine.BatchMatcher(eng) for _ in range(R)]
        self.sess = [engine.VehicleSessions(bm, n_vehicles, report_dist_m=ss.PARAMS["dist"], report_count=ss.PARAMS["count"],
                                            report_time_s=ss.PARAMS["time_s"]) for bm in self.bms]
        self.dirs = [engine.VehicleDirectory(n_vehicles) for _ in range(R)]
        self.stores = [engine.TileStore(0, ss.Q, ss.PRIVACY, initial_rows=rows0) for _ in range(R)]
        self.windows, self.flushes = [], []

    def close(self):
        for x in self.stores + self.dirs + self.sess + self.bms:
            x.close()

    def poll(self, text):
        w = []
        for r in range(self.R):
            self.sess[r].push_messages([text], FMT(), self.dirs[r], shard=(r, self.R) if self.sharded else None)
            self.stores[r].add_session(self.sess[r])
            w.append(self.sess[r].windows().copy())
        self.windows.append(w)

    def punctuate(self, ts):
        w = []
        for r in range(self.R):
            self.sess[r].punctuate(ts)
            self.stores[r].add_session(self.sess[r])
            w.append(self.sess[r].windows().copy())
        self.windows.append(w)

    def flush(self):
        if self.sharded:
            blobs = [s.export_rows() for s in self.stores]
            for r, s in enumerate(self.stores):
                s.import_owned(blobs, r, self.R)
        self.flushes.append([s.flush()[0] for s in self.stores])

    def run(self, sc, first, last):
        """Polls first .. last - 1 with the scenario's flushes; behind the last poll of all, the punctuate and its flush."""
        for k in range(first, last):
            self.poll(sc["texts"][k])
            if k in sc["flush_after"]:
                self.flush()
        if last == len(sc["texts"]):
            self.punctuate(sc["ts"])
            self.flush()

    def save(self, user=b""):
        if not self.sharded:
            return [engine.save_stream(self.sess[0], self.dirs[0], self.stores[0], user)]
        return [engine.save_stream_shard(self.sess[r], self.dirs[r], self.stores[r], (r, self.R), user) for r in range(self.R)]

    def load(self, blobs):
        return [engine.load_stream_shards(blobs, self.sess[r], self.dirs[r], self.stores[r], shard=(r, self.R)) for r in range(self.R)]


def _merged(per_rank):
    w = np.concatenate(per_rank)
    return w[np.argsort(w["arrival"], kind="stable")]


@pytest.fixture(scope="module")
def runs(built_lib, small_world):
    sc = ss.scenario(small_world)
    stop = sh.choose_stop(small_world)
    n = sc["n_vehicles"]
    eng = engine.Engine(small_world, 0)
    out = {"sc": sc, "stop": stop, "eng": eng, "saved": {}, "early": {}, "cont": {}}
    try:
        one = Ranks(eng, 1, n, sharded=False)
        try:
            one.run(sc, 0, len(sc["texts"]))
            out["one"] = {"flushes": [f[0] for f in one.flushes], "windows": [w[0] for w in one.windows], "names": one.dirs[0].names()}
        finally:
            one.close()
        for M in (1, 2, 3):
            rk = Ranks(eng, M, n, sharded=M > 1)
            try:
                if M == 2:
                    out["early"] = rk.save()   # the same ranks at another stop: before the first poll
                rk.run(sc, 0, stop)
                out["saved"][M] = rk.save(b"stop %d" % stop)
                out["saved_flushes"] = len(rk.flushes)
            finally:
                rk.close()                     # everything is torn down before anything is loaded
        for M, N in PAIRS:
            # other sizes on the loading side, and for one pair another hash mask: the table is rebuilt
            nv = {(2, 3): n + 16, (3, 2): n + 1}.get((M, N), n)
            if (M, N) == (2, 3):
                os.environ["RM_LINES_HASH_BITS"] = "4"
            rk = Ranks(eng, N, nv, rows0=1 if N == 3 else 64)
            try:
                counts = rk.load(out["saved"][M])
                again = rk.save()
                after_load = [(len(rk.sess[r].reports()), len(rk.sess[r].windows())) for r in range(N)]
                rk.run(sc, stop, len(sc["texts"]))
                out["cont"][(M, N)] = {"counts": counts, "again": again, "after_load": after_load, "flushes": rk.flushes,
                                       "windows": rk.windows, "names": [d.names() for d in rk.dirs]}
            finally:
                rk.close()
                os.environ.pop("RM_LINES_HASH_BITS", None)
        yield out
    finally:
        eng.close()


@pytest.mark.parametrize("M,N", PAIRS)
def test_resumed_on_n_ranks_writes_the_one_rank_files(runs, M, N):
    sc, stop, one, got = runs["sc"], runs["stop"], runs["one"], runs["cont"][(M, N)]
    done = runs["saved_flushes"]                     # flushes before the stop
    later = one["flushes"][done:]
    assert len(got["flushes"]) == len(later) >= 1 and all(len(f) > 0 for f in later)
    for want, per_rank in zip(later, got["flushes"]):
        union = {}
        for r, files in enumerate(per_rank):
            assert not set(files) & set(union)       # each file is written by one rank
            union.update(files)
            for name in files:                       # ... the one rm_tile_file_owner names
                span, level, index = name.split("/")
                assert engine.tile_file_owner(int(span.split("_")[0]) // ss.Q, int(level) | int(index) << 3, N) == r
        assert union == dict(want)
    # the model's continued files, rank by rank
    mfiles = sh.resume(sc["path"], M, N, stop)["files"]
    assert [[dict(f) for f in per_rank] for per_rank in got["flushes"]] == [[dict(f) for f in per_rank] for per_rank in mfiles]
    # the windows of every later call, merged by arrival, and the names
    want_w = one["windows"][stop:]
    assert len(got["windows"]) == len(want_w) and sum(len(w) for w in want_w) > 0
    for want, per_rank in zip(want_w, got["windows"]):
        for r, w in enumerate(per_rank):
            assert all(ss.vehicle_owner(int(v), N) == r for v in w["vehicle"])
        assert _merged(per_rank).tobytes() == want.tobytes()
    assert all(x == one["names"] for x in got["names"])
    assert got["after_load"] == [(0, 0)] * N         # the last call's outputs are not state


@pytest.mark.parametrize("M,N", PAIRS)
def test_a_save_after_the_load_holds_the_models_resharded_state(runs, M, N):
    sc, stop, got = runs["sc"], runs["stop"], runs["cont"][(M, N)]
    model = sh.resume(sc["path"], M, N, stop)
    calls = model["saved"][0]["calls"]
    assert sum(len(rows) for _, rows in model["loaded"]) > 0 and all(len(recs) > 0 for recs, _ in model["loaded"])
    for r in range(N):
        info = engine.snapshot_info(got["again"][r])
        assert (info["rank"], info["nranks"], info["calls"]) == (r, N, calls)
        recs, rows = sh.blob_state(got["again"][r])
        want_recs, want_rows = model["loaded"][r]
        assert recs == want_recs
        assert rows == want_rows
        c = got["counts"][r]
        assert (c["vehicles"], c["rows"], c["calls"], c["saved_ranks"]) == (len(want_recs), len(want_rows), calls, M)
        assert c["points"] == sum(x[1] for x in want_recs) and c["names"] == info["names"] > 0
    # what was saved is the model's too (the plain blob carries no keys: blob_state numbers its rows)
    for b, blob in zip(model["saved"], runs["saved"][M]):
        info = engine.snapshot_info(blob)
        assert info["user"] == b"stop %d" % stop and ("nranks" in info) == (M > 1)
        recs, rows = sh.blob_state(blob)
        assert [x[0] for x in recs] == [v for v, _ in b["records"]]
        assert rows == [sh.row_tuple(*row) for row in b["rows"]]


def _fresh(runs, N=2, nv=None):
    bm = engine.BatchMatcher(runs["eng"])
    n = nv or runs["sc"]["n_vehicles"]
    s = engine.VehicleSessions(bm, n, report_dist_m=ss.PARAMS["dist"], report_count=ss.PARAMS["count"], report_time_s=ss.PARAMS["time_s"])
    return [bm, s, engine.VehicleDirectory(n), engine.TileStore(0, ss.Q, ss.PRIVACY, initial_rows=8)]


def _blob_with(blob, edit):
    secs, _ = sn.read(blob)
    edit(secs)
    return sh.write(secs)


def test_broken_sets_are_refused_and_leave_the_objects_usable(runs):
    sc, stop = runs["sc"], runs["stop"]
    good = runs["saved"][2]
    want = sh.resume(sc["path"], 2, 2, stop)["loaded"][0]
    _, table = sn.read(good[1])
    koff = next(e[2] for e in table if e[0] == sh.TILE_KEYS)
    assert next(e[3] for e in table if e[0] == sh.TILE_KEYS) > 0
    flipped = bytearray(good[1])
    flipped[koff + 2] ^= 0x04

    def sessions_of_rank0(secs):
        other, _ = sn.read(good[0])
        for k in (sn.SESS_REC, sn.SESS_LON, sn.SESS_LAT, sn.SESS_ACC, sn.SESS_TIME):
            secs[k] = other[k]
    cases = [
        ([good[0]], "2 ranks, and 1 blobs are given"),                       # one blob of the set missing
        ([good[0], good[0]], "rank 0 of the save is given twice"),           # one blob given twice
        ([good[0], runs["early"][1]], "different stops"),                    # blobs of two different stops
        ([good[0], bytes(flipped)], "a section's checksum does not match"),  # one flipped bit in a key section
        ([good[0], _blob_with(good[1], sessions_of_rank0)], "a vehicle's session is in two blobs"),
    ]
    for blobs, msg in cases:
        objs = _fresh(runs)
        try:
            with pytest.raises(_lib.RmError, match=msg):
                engine.load_stream_shards(blobs, *objs[1:], shard=(0, 2))
            assert objs[2].size == 0 and objs[1].store()["cnt"].sum() == 0 and objs[3].flush()[1]["rows_in"] == 0
            # empty and usable: the good set goes in, and a save holds the model's state
            engine.load_stream_shards(list(reversed(good)), *objs[1:], shard=(0, 2))   # (in any order)
            assert sh.blob_state(engine.save_stream_shard(*objs[1:], shard=(0, 2))) == want
        finally:
            for o in reversed(objs):
                o.close()


def _tree(d):
    out = {}
    for root, _, fs in os.walk(d):
        for f in fs:
            p = os.path.join(root, f)
            out[os.path.relpath(p, d)] = open(p, "rb").read()
    return out


def test_cli_stops_on_two_ranks_and_resumes_on_three(built_lib, small_world, tmp_path):
    """python -m reporter_amd.stream in fresh child processes: an unbroken one-rank run; a stop on two
    ranks; a resume that finds a rank file missing; the resume on three ranks."""
    sc = ss.scenario(small_world)
    src = tmp_path / "in"
    src.mkdir()
    (src / "a.txt").write_bytes(b"".join(sc["texts"]))
    conf = tmp_path / "conf.json"
    conf.write_text(json.dumps({"meili": {"default": {}}, "reporter_amd": {"graph": small_world}}))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), RM_RDZV_DIR=str(tmp_path),
               RM_COMM_TIMEOUT_S="120")

    def cli(out, *more):
        return subprocess.run(["timeout", "-k", "10", "280", sys.executable, "-m", "reporter_amd.stream", "--formatter", "@sv@,@0@2@3@1@4",
                               "--match-config", str(conf), "--output-location", str(out), "--privacy", str(ss.PRIVACY),
                               "--quantisation", str(ss.Q), "--flush-interval", "150", "--max-vehicles", str(sc["n_vehicles"]),
                               "--poll-bytes", "32768", "--report-dist", str(ss.PARAMS["dist"]), "--report-count", str(ss.PARAMS["count"]),
                               "--report-time", str(ss.PARAMS["time_s"]), str(src)] + list(more),
                              capture_output=True, text=True, env=env)

    stats = lambda r: json.loads(r.stdout.strip().splitlines()[-1])
    r = cli(tmp_path / "one")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    one = stats(r)
    assert one["flushes"] >= 3 and one["polls"] >= 4 and one["forwarded"] > 0 and one["files"] > 0
    ck = str(tmp_path / "ck")
    r = cli(tmp_path / "parts", "--ranks", "2", "--transport", "host", "--checkpoint", ck, "--stop-after-polls", "3")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    first = stats(r)
    assert first["polls"] == 3 and first.get("stopped") and 0 < first["messages"] < one["messages"]
    head = json.loads(engine.snapshot_info(open(ck, "rb").read())["user"].decode())
    assert head["ranks"] == 2 and head["generation"] >= 1 and not head["done"]
    files = sorted(f for f in os.listdir(tmp_path) if f.startswith("ck"))
    assert files == ["ck"] + ["ck.g%d.r%d" % (head["generation"], k) for k in range(2)]   # one generation, no leftovers
    infos = [engine.snapshot_info(open(tmp_path / f, "rb").read()) for f in files[1:]]
    assert [(i["rank"], i["nranks"]) for i in infos] == [(0, 2), (1, 2)] and infos[0]["calls"] == infos[1]["calls"] == 3
    print("stopped with", [(i["vehicles"], i["points"], i["rows"]) for i in infos], "vehicles, points, rows")
    assert all(i["vehicles"] > 0 for i in infos)   # open sessions on both ranks
    # a copy of the checkpoint with one rank file missing: the resume refuses and writes nothing
    bad = tmp_path / "bad"
    bad.mkdir()
    (bad / "ck").write_bytes(open(ck, "rb").read())
    (bad / files[1]).write_bytes(open(tmp_path / files[1], "rb").read())
    r = cli(tmp_path / "x", "--ranks", "3", "--transport", "host", "--checkpoint", str(bad / "ck"), "--resume")
    assert r.returncode != 0 and "is missing" in r.stderr
    assert not os.path.exists(tmp_path / "x") or not _tree(tmp_path / "x")
    # the resume on three ranks
    r = cli(tmp_path / "parts", "--ranks", "3", "--transport", "host", "--checkpoint", ck, "--resume")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert stats(r) == one
    assert _tree(tmp_path / "parts") == _tree(tmp_path / "one") and len(_tree(tmp_path / "one")) > 0
    head = json.loads(engine.snapshot_info(open(ck, "rb").read())["user"].decode())
    assert head["ranks"] == 3 and head["done"] is True
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("ck")) == ["ck"] + ["ck.g%d.r%d" % (head["generation"], k) for k in range(3)]


def test_the_pinned_refusals_still_refuse(runs):
    good, plain = runs["saved"][2], runs["saved"][1][0]
    objs = _fresh(runs)
    other = _fresh(runs)
    try:
        engine.load_stream_shards(good, *objs[1:], shard=(1, 2))
        with pytest.raises(_lib.RmError, match="row keys"):                   # rm_snapshot_save of a keyed store
            engine.save_stream(*objs[1:])
        with pytest.raises(_lib.RmError, match="rm_snapshot_load_shards"):   # rm_snapshot_load of kinds 11 / 12
            engine.load_stream(good[0], *other[1:])
        objs[3].flush()
        with pytest.raises(_lib.RmError, match="keeps row keys"):            # rm_snapshot_load into a keyed store
            engine.load_stream(plain, store=objs[3])
        engine.load_stream(plain, *other[1:])
        with pytest.raises(_lib.RmError, match="restored from a snapshot"):  # make_keyed on rows the plain load restored
            other[3].export_rows()
        assert "nranks" not in engine.snapshot_info(plain) and len(sn.read(plain)[1]) == 10   # the plain blob is today's
    finally:
        for o in reversed(objs + other):
            o.close()
