"""Stream formatter probe (rule 14): C2's workload as raw messages into vehicle sessions,
by the device route and by the route the host arrays offered before it.

    python scripts/stream_probe.py [--vehicles 10000] [--points 600] [--per-push 60] [--runs 4]
                                   [--out profiles/stream/stream_probe.json]

The vehicles' traces are written as text in time order, --per-push messages per vehicle in a push
(10,000 x 60: 600 k messages), once as separated values and once as JSON.  Route (a) is
VehicleSessions.push_messages: one upload of the text, everything else on the device; its split is
rm_session_messages_time's.  Route (b) is what the same bytes took before: BatchMatcher.parse_lines,
the download of the points and the names, a Python dictionary from name to persistent index, then
VehicleSessions.push with host arrays.  (b) reads separated values only: there was no such route
for JSON text, so JSON is timed by (a) alone.  The routes alternate --runs times in one process
after a warm-up push of each.  Prints one JSON line and writes it to --out.

    python scripts/stream_probe.py --snapshot-at 5 [--out profiles/snapshot/snapshot_probe.json]

instead measures the stream snapshot (rule 15) on the separated-value messages: the whole topology
(directory, sessions, tile store) runs unbroken, then again with a save after push K, new objects, a
load, and the remaining pushes; the outputs of the pushes behind K and the hash of the flushed files
must equal the unbroken run's.  Reported: the blob's bytes per section, the save and load parts (HIP
events, after one warm-up save and load), the checksum kernel's bytes/s, and beside them the only
read-out there was before, VehicleSessions.store() plus VehicleDirectory.names() on the same state.

    python scripts/stream_probe.py --snapshot-shard-at 5 [--out profiles/snapshot_shard/snapshot_shard_probe.json]

measures the sharded snapshot (rule 17) beside the plain one: two ranks sharing this GPU and process,
saved after push K, loaded on two ranks and on three, the calls alternating; the loaded sets go on to
the end and must flush the unbroken run's files."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from reporter_amd import engine, world   # noqa: E402

PARTS = ("text_upload", "parse", "ids", "directory", "upload", "append", "trigger", "match", "trim")


def write_text(arr, a, b, kind):
    v, t, la, lo, ac = arr["vehicle"][a:b], arr["time"][a:b], arr["lat"][a:b], arr["lon"][a:b], arr["accuracy"][a:b]
    if kind == 0:
        rows = ["veh-%07d,%d,%.6f,%.6f,%.1f" % r for r in zip(v.tolist(), t.astype(np.int64).tolist(), la.tolist(), lo.tolist(),
                                                               ac.tolist())]
    else:
        rows = ['{"id":"veh-%07d","timestamp":%d,"latitude":%.6f,"longitude":%.6f,"accuracy":%.1f}' % r
                for r in zip(v.tolist(), t.astype(np.int64).tolist(), la.tolist(), lo.tolist(), ac.tolist())]
    return ("\n".join(rows) + "\n").encode()


def route_a(bm, texts, fmt, n_vehicles):
    sess = engine.VehicleSessions(bm, n_vehicles)
    vdir = engine.VehicleDirectory(n_vehicles)
    pushes, msgs, host_lines, lines, fwd = [], 0, 0, 0, 0
    for text in texts:
        t0 = time.perf_counter()
        out, info = sess.push_messages([text], fmt, vdir)
        wall = (time.perf_counter() - t0) * 1e3
        ms = sess.messages_ms()
        pushes.append([round(wall, 3)] + [round(ms[p], 3) for p in PARTS])
        msgs += info["points"]
        host_lines += info["host_lines"]
        lines += info["lines"]
        fwd += out["forwarded"]
    size = vdir.size
    vdir.close()
    sess.close()
    p = np.array(pushes)
    wall_s = p[:, 0].sum() * 1e-3
    return dict(wall_s=wall_s, messages=msgs, messages_per_s=msgs / wall_s, forwarded=fwd, vehicles=size,
                host_line_share=host_lines / max(lines, 1), sum_ms=dict(zip(("wall",) + PARTS, p.sum(axis=0).round(2).tolist())),
                push_columns=["wall_ms"] + list(PARTS), pushes=pushes)


def route_b(bm, texts, n_vehicles):
    sess = engine.VehicleSessions(bm, n_vehicles)
    table = {}
    pushes, msgs, fwd = [], 0, 0
    for text in texts:
        t0 = time.perf_counter()
        pts = bm.parse_lines([text])
        t1 = time.perf_counter()
        names = bm.vehicle_names([text])
        lut = np.empty(len(names), np.uint32)
        for k, name in enumerate(names):
            lut[k] = table.setdefault(name, len(table))
        idx = lut[pts["uuid"]]
        t2 = time.perf_counter()
        out = sess.push(idx, pts["time"], pts["lon"], pts["lat"], pts["accuracy"], (pts["time"] * 1000.0).astype(np.int64))
        t3 = time.perf_counter()
        pushes.append([round((t3 - t0) * 1e3, 3), round((t1 - t0) * 1e3, 3), round((t2 - t1) * 1e3, 3), round((t3 - t2) * 1e3, 3)])
        msgs += len(idx)
        fwd += out["forwarded"]
    sess.close()
    p = np.array(pushes)
    wall_s = p[:, 0].sum() * 1e-3
    cols = ("wall", "parse_and_download", "names_and_dictionary", "push")
    return dict(wall_s=wall_s, messages=msgs, messages_per_s=msgs / wall_s, forwarded=fwd, vehicles=len(table),
                sum_ms=dict(zip(cols, p.sum(axis=0).round(2).tolist())), push_columns=[c + "_ms" for c in cols], pushes=pushes)


SECTION_NAMES = {1: "user", 2: "name_offsets", 3: "name_bytes", 4: "session_records", 5: "lon", 6: "lat", 7: "accuracy",
                 8: "time", 9: "tile_rows", 10: "tile_numbers"}


def snapshot_probe(bm, texts, fmt, n_vehicles, at):
    import hashlib
    import struct
    digest = lambda *xs: hashlib.sha256(b"".join(xs)).hexdigest()
    make = lambda: (engine.VehicleSessions(bm, n_vehicles), engine.VehicleDirectory(n_vehicles), engine.TileStore(0))

    def pushes(objs, first, last):
        out = []
        for text in texts[first:last]:
            objs[0].push_messages([text], fmt, objs[1])
            objs[2].add_session(objs[0])
            out.append(digest(objs[0].windows().tobytes(), objs[0].reports().tobytes()))
        return out

    def finish(objs):
        files, counts = objs[2].flush()
        names = digest(*(n.encode() for n in objs[1].names()))
        for o in reversed(objs):
            o.close()
        return digest(*(k.encode() + b"\0" + v for k, v in files.items())), counts, names

    objs = make()
    want = pushes(objs, 0, len(texts))
    want_end = finish(objs)
    print("unbroken run done", file=sys.stderr, flush=True)
    objs = make()
    head = pushes(objs, 0, at)
    scratch = make()                      # one warm-up save and load
    engine.load_stream(engine.save_stream(*objs), *scratch)
    for o in reversed(scratch):
        o.close()
    save_runs, load_runs = [], []
    for _ in range(5):                    # a save changes nothing: the same state, five times
        t0 = time.perf_counter()
        blob = engine.save_stream(*objs, user=b"stream_probe")
        save_runs.append(dict(engine.save_stream.last["ms"], wall=(time.perf_counter() - t0) * 1e3))
    saved = dict(engine.save_stream.last)
    for _ in range(4):                    # ... and four loads into objects made for it, before the one that goes on
        scratch = make()
        t0 = time.perf_counter()
        got = engine.load_stream(blob, *scratch)
        load_runs.append(dict(got["ms"], wall=(time.perf_counter() - t0) * 1e3))
        for o in reversed(scratch):
            o.close()
    t0 = time.perf_counter()              # what there was before: two read-outs, no restore, no tile rows
    st = objs[0].store()
    t1 = time.perf_counter()
    names = objs[1].names()
    t2 = time.perf_counter()
    for o in reversed(objs):
        o.close()
    objs = make()
    t3 = time.perf_counter()
    loaded = engine.load_stream(blob, *objs)
    load_runs.append(dict(loaded["ms"], wall=(time.perf_counter() - t3) * 1e3))
    tail = pushes(objs, at, len(texts))
    end = finish(objs)
    n_sec = struct.unpack_from("<I", blob, 12)[0]
    sections = {}
    for k in range(n_sec):
        kind, _, _, nbytes, _, _ = struct.unpack_from("<IIQQQQ", blob, 32 + 40 * k)
        sections[SECTION_NAMES.get(kind, str(kind))] = nbytes
    summed = sum(sections.values())
    return dict(snapshot_at=at, pushes=len(texts), outputs_equal=head + tail == want, flush_equal=end == want_end,
                flush_sha256=end[0], flush_counts=end[1], blob_bytes=len(blob), section_bytes=sections,
                counts={k: v for k, v in saved.items() if k != "ms"}, save_ms_runs=save_runs, load_ms_runs=load_runs,
                checksum_bytes_per_s=[summed / (r["checksum"] * 1e-3) if r["checksum"] > 0 else None for r in save_runs],
                peak_bytes_per_s=8e12,
                before=dict(store_wall_ms=(t1 - t0) * 1e3, names_wall_ms=(t2 - t1) * 1e3, points=len(st["lon"]), names=len(names),
                            note="VehicleSessions.store() + VehicleDirectory.names(): read-outs only, no tile rows, nothing loads them"))


def snapshot_shard_probe(eng, texts, fmt, n_vehicles, at, runs=5):
    """Rule 17 beside rule 15 on one state: the stream runs unbroken on one rank, then to push `at`
    once on one rank and once on two ranks sharing this GPU and process (the exchange by export /
    import).  After a warm-up of each kind, `runs` rounds alternate: the plain save and load, the
    two ranks' shard saves, the loads of the two blobs on two ranks and on three.  The two- and
    three-rank loads of the last round go on to the end; their files must be the unbroken run's."""
    import hashlib
    digest = lambda files: hashlib.sha256(b"".join(k.encode() + b"\0" + v for k, v in sorted(files.items()))).hexdigest()

    def make(R):
        bms = [engine.BatchMatcher(eng) for _ in range(R)]
        return [(bm, engine.VehicleSessions(bm, n_vehicles), engine.VehicleDirectory(n_vehicles), engine.TileStore(0)) for bm in bms]

    def close(sets):
        for s in sets:
            for o in reversed(s):
                o.close()

    def pushes(sets, first, last, sharded):
        R = len(sets)
        for text in texts[first:last]:
            for r, (_, sess, vdir, store) in enumerate(sets):
                sess.push_messages([text], fmt, vdir, shard=(r, R) if sharded else None)
                store.add_session(sess)

    def finish(sets, sharded):
        if sharded:
            blobs = [s[3].export_rows() for s in sets]
            for r, s in enumerate(sets):
                s[3].import_owned(blobs, r, len(sets))
        files = {}
        for s in sets:
            got = s[3].flush()[0]
            assert not set(got) & set(files)
            files.update(got)
        return digest(files), len(files)

    timed = lambda f: (lambda t0, r: (r, (time.perf_counter() - t0) * 1e3))(time.perf_counter(), f())
    one = make(1)
    pushes(one, 0, len(texts), False)
    want = finish(one, False)
    close(one)
    print("unbroken run done", file=sys.stderr, flush=True)
    one, two = make(1), make(2)
    pushes(one, 0, at, False)
    pushes(two, 0, at, True)
    print("states at push %d ready" % at, file=sys.stderr, flush=True)

    def save_plain():
        blob, wall = timed(lambda: engine.save_stream(*one[0][1:], user=b"stream_probe"))
        return blob, dict(engine.save_stream.last["ms"], wall=wall, bytes=len(blob))

    def save_shard(r):
        blob, wall = timed(lambda: engine.save_stream_shard(*two[r][1:], shard=(r, 2), user=b"stream_probe"))
        return blob, dict(engine.save_stream_shard.last["ms"], wall=wall, bytes=len(blob))

    def load_plain(blob):
        s = make(1)
        got, wall = timed(lambda: engine.load_stream(blob, *s[0][1:]))
        close(s)
        return dict(got["ms"], wall=wall)

    def load_shards(blobs, N, keep=False):
        sets, out = make(N), []
        for r in range(N):
            got, wall = timed(lambda: engine.load_stream_shards(blobs, *sets[r][1:], shard=(r, N)))
            out.append(dict(got["ms"], wall=wall, held=dict(vehicles=got["vehicles"], points=got["points"], rows=got["rows"])))
        if keep:
            return out, sets
        close(sets)
        return out, None

    plain, _ = save_plain()             # one warm-up of each kind
    shards = [save_shard(r)[0] for r in range(2)]
    load_plain(plain)
    load_shards(shards, 2)
    load_shards(shards, 3)
    rounds = []
    for k in range(runs):
        rd = {}
        plain, rd["plain_save"] = save_plain()
        saves = [save_shard(r) for r in range(2)]
        shards, rd["shard_save"] = [b for b, _ in saves], [m for _, m in saves]
        rd["plain_load"] = load_plain(plain)
        rd["shard_load_2_to_2"], keep2 = load_shards(shards, 2, keep=k + 1 == runs)
        rd["shard_load_2_to_3"], keep3 = load_shards(shards, 3, keep=k + 1 == runs)
        rounds.append(rd)
    close(one)
    close(two)
    ends = {}
    for name, sets in (("2_to_2", keep2), ("2_to_3", keep3)):
        pushes(sets, at, len(texts), True)
        ends[name] = finish(sets, True)
        close(sets)
    infos = [engine.snapshot_info(b) for b in [plain] + shards]
    return dict(snapshot_at=at, pushes=len(texts), flush_sha256=want[0], files=want[1],
                continued_equal={k: v == want for k, v in ends.items()},
                blobs=[{k: i.get(k) for k in ("bytes", "names", "vehicles", "points", "rows", "rank", "nranks", "calls")} for i in infos],
                rounds=rounds, note="two ranks sharing one GPU and process: the calls' cost, not scaling")


def sharded_probe(bm, texts, fmt, n_vehicles, comm, flush_every):
    """The stream of rule 16 on this rank: masked pushes, the tile store fed device to device, and every
    `flush_every` pushes (and at the end) the exchange and a flush.  Per flush the exchange's three stage
    times (HIP events) and its row counts; per push the route's parts as route_a gives them."""
    sess = engine.VehicleSessions(bm, n_vehicles)
    vdir = engine.VehicleDirectory(n_vehicles)
    store = engine.TileStore(comm.device)
    shard = (comm.rank, comm.world_size)
    pushes, flushes, own = [], [], 0
    for k, text in enumerate(texts):
        t0 = time.perf_counter()
        out, info = sess.push_messages([text], fmt, vdir, shard=shard)
        wall = (time.perf_counter() - t0) * 1e3
        ms = sess.messages_ms()
        store.add_session(sess)
        pushes.append([round(wall, 3)] + [round(ms[p], 3) for p in PARTS])
        own += info["own"]
        if (k + 1) % flush_every == 0 or k + 1 == len(texts):
            t0 = time.perf_counter()
            moved = store.exchange(comm)
            wall = (time.perf_counter() - t0) * 1e3
            files, counts = store.flush()
            flushes.append(dict(moved, wall_ms=round(wall, 3), files=counts["files"],
                                **{k2: round(v, 4) for k2, v in store.exchange_ms().items()}))
    for x in (store, vdir, sess):
        x.close()
    p = np.array(pushes)
    return dict(rank=comm.rank, ranks=comm.world_size, own_points=own, sum_ms=dict(zip(("wall",) + PARTS, p.sum(axis=0).round(2).tolist())),
                push_columns=["wall_ms"] + list(PARTS), pushes=pushes, flushes=flushes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vehicles", type=int, default=10000)
    ap.add_argument("--points", type=int, default=600)
    ap.add_argument("--per-push", type=int, default=60)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--snapshot-at", type=int, help="measure the stream snapshot: save after this push, load, finish")
    ap.add_argument("--snapshot-shard-at", type=int, help="measure the sharded snapshot (rule 17) beside the plain one: two "
                    "ranks sharing this GPU, saved after this push, loaded on two and on three ranks")
    ap.add_argument("--out")
    ap.add_argument("--ranks", type=int, default=1, help="the stream of DESIGN.md §3 rule 16 on this many ranks (one fresh "
                    "process each): per flush the exchange's stage times and rows moved, one JSON file per rank")
    ap.add_argument("--transport", choices=("rccl", "host"), default="rccl", help="host: gloo, so the ranks can share one GPU")
    ap.add_argument("--flush-every", type=int, default=2, help="with --ranks: pushes between two flushes")
    a = ap.parse_args()
    ranked = "RANK" in os.environ and int(os.environ.get("WORLD_SIZE", "1")) > 1
    if a.ranks > 1 and not ranked:
        from reporter_amd import dist
        env_path = os.pathsep.join([os.path.join(ROOT, "scripts"), ROOT, os.environ.get("PYTHONPATH", "")])
        os.environ["PYTHONPATH"] = env_path
        sys.exit(dist.self_launch("stream_probe", sys.argv[1:], a.ranks))
    a.out = a.out or (os.path.join("profiles", "snapshot", "snapshot_probe.json") if a.snapshot_at is not None
                      else os.path.join("profiles", "snapshot_shard", "snapshot_shard_probe.json") if a.snapshot_shard_at is not None
                      else os.path.join("profiles", "stream", "stream_probe.json"))
    cfg = world.CONFIGS["C2"]
    tmp = tempfile.mkdtemp(prefix="stream_probe")
    graph = os.path.join(tmp, "c2.rmg")
    world.build_world(graph, cfg["rows"], cfg["cols"], cfg["block_m"], seed=1, cell_m=cfg["cell_m"])
    tr = world.generate_traces(graph, n_traces=a.vehicles, n_points=a.points, rate_s=cfg["rate_s"], noise_m=cfg["noise_m"],
                               seed=1000)
    T, n = a.vehicles, a.points
    order = np.arange(T * n).reshape(T, n).T.ravel()          # time-major: every vehicle's k-th point, then the next
    arr = {"vehicle": (order // n).astype(np.uint32)}
    for f in ("time", "lon", "lat", "accuracy"):
        arr[f] = np.ascontiguousarray(tr[f][order])
    per = a.per_push * T
    cuts = [(s, min(s + per, T * n)) for s in range(0, T * n, per)]
    sv_only = a.snapshot_at is not None or a.snapshot_shard_at is not None
    texts = {kind: [write_text(arr, s, e, kind) for s, e in cuts] for kind in ((0,) if sv_only else (0, 1))}
    fmt = {0: engine.MessageFormat(0), 1: engine.MessageFormat(1)}
    device = 0
    if ranked:   # each rank its own GPU, as python -m reporter_amd.stream takes them; only the host transport may share one
        import ctypes
        from reporter_amd import _lib
        cnt = ctypes.c_int(0)
        _lib.check(_lib.lib().rm_device_count(ctypes.byref(cnt)))
        if a.transport == "rccl" and int(os.environ["WORLD_SIZE"]) > max(cnt.value, 1):
            sys.exit("--transport rccl needs a GPU per rank (%d ranks, %d devices): use --transport host" %
                     (int(os.environ["WORLD_SIZE"]), cnt.value))
        device = int(os.environ.get("LOCAL_RANK", "0")) % max(cnt.value, 1)
    eng = engine.Engine(graph, device)
    bm = engine.BatchMatcher(eng)
    if ranked:
        from reporter_amd import dist
        rank, world_size = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
        comm = dist.stream_comm(rank, world_size, device, a.transport)
        route_a(bm, texts[0][:2], fmt[0], T)   # warm the route
        out = dict(args=dict(vehicles=a.vehicles, points=a.points, per_push=a.per_push, ranks=world_size, transport=a.transport,
                             flush_every=a.flush_every), messages_per_push=per,
                   note="ranks sharing one GPU show the exchange's cost, not scaling",
                   **sharded_probe(bm, texts[0], fmt[0], T, comm, a.flush_every))
        comm.close()
        path = (a.out if a.out.endswith(".json") and "stream_probe.json" not in a.out else
                os.path.join("profiles", "stream_shard", "stream_probe.json"))[:-5] + ".rank%d.json" % rank
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "w") as f:
            f.write(json.dumps(out) + "\n")
        if rank == 0:
            print(json.dumps(dict(out, pushes=None)))
        bm.close()
        eng.close()
        return
    if a.snapshot_shard_at is not None:
        print("text written", file=sys.stderr, flush=True)
        route_a(bm, texts[0][:2], fmt[0], T)   # warm the route
        out = dict(args=dict(vehicles=a.vehicles, points=a.points, per_push=a.per_push, snapshot_shard_at=a.snapshot_shard_at),
                   messages_per_push=per, **snapshot_shard_probe(eng, texts[0], fmt[0], T, a.snapshot_shard_at))
        line = json.dumps(out)
        print(line)
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
        bm.close()
        eng.close()
        return
    if a.snapshot_at is not None:
        print("text written", file=sys.stderr, flush=True)
        route_a(bm, texts[0][:2], fmt[0], T)   # warm the route
        out = dict(args=dict(vehicles=a.vehicles, points=a.points, per_push=a.per_push, snapshot_at=a.snapshot_at),
                   messages_per_push=per, **snapshot_probe(bm, texts[0], fmt[0], T, a.snapshot_at))
        line = json.dumps(out)
        print(line)
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
        bm.close()
        eng.close()
        return
    # warm every route (route tables, workspaces, the readers' buffers)
    route_a(bm, texts[0][:2], fmt[0], T)
    route_a(bm, texts[1][:2], fmt[1], T)
    route_b(bm, texts[0][:2], T)
    runs = []
    for _ in range(max(a.runs, 1)):
        runs.append(dict(a_sv=route_a(bm, texts[0], fmt[0], T), b_sv=route_b(bm, texts[0], T),
                         a_json=route_a(bm, texts[1], fmt[1], T)))
    out = dict(args=dict(vehicles=a.vehicles, points=a.points, per_push=a.per_push, runs=a.runs),   # the invocation
               vehicles=T, points_per_vehicle=n, messages_per_push=per, pushes=len(cuts),
               text_bytes=dict(sv=sum(len(t) for t in texts[0]), json=sum(len(t) for t in texts[1])), runs=runs,
               a_sv_messages_per_s=[r["a_sv"]["messages_per_s"] for r in runs],
               b_sv_messages_per_s=[r["b_sv"]["messages_per_s"] for r in runs],
               a_json_messages_per_s=[r["a_json"]["messages_per_s"] for r in runs],
               note="(b) has no JSON route: a_json stands beside b_sv only as the same messages in another spelling")
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    bm.close()
    eng.close()


if __name__ == "__main__":
    main()
