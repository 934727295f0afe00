"""GPU stream reporter: the reference's streaming topology (Reporter.java: formatter -> batcher ->
anonymiser) over files of raw messages, every processor on the MI355X.

    python -m reporter_amd.stream --formatter '@json@id@lat@lon@time@acc' --match-config conf.json \\
        --output-location out/ messages.txt [more files or directories ...]

The text goes up in polls of about --poll-bytes; each poll is read, keyed through the vehicle
directory and pushed into the vehicle sessions on the device (rm_session_push_messages), and the
forwarded reports join the tile store device to device.  Stream time is the messages' own: whenever
it has advanced --flush-interval seconds past the last flush the tile store is flushed, and once at
the end, after a punctuate that evicts every vehicle.  Tiles are written under --output-location as
reporter_amd.batch writes them; a tile flushed again later gets the suffix ".<flush number>".

With --checkpoint FILE the stream's state (sessions, directory, tile store: DESIGN.md §3 rule 15) and
its position in the input are written to FILE after every tile flush and at a stop;
--stop-after-polls N stops after N polls without the final punctuate and flush (the file-fed
counterpart of Reporter.java --duration), and --resume continues from FILE, writing what the
stream that never stopped would have written.

With --ranks N the stream runs on N GPUs (DESIGN.md §3 rule 16) and writes, file for file and byte
for byte, what one rank writes: N fresh child processes are started, one per rank (or the ranks come
from torch.distributed.run through RANK / WORLD_SIZE / LOCAL_RANK); every rank reads and keys all
the text, holds the sessions of the vehicles it owns, and before each flush the tile rows go to the
rank that owns their file, which alone writes it.  --transport host carries the exchange over gloo,
so several ranks can share one GPU (rank r takes GPU LOCAL_RANK modulo the device count).  Rank 0
prints the summed statistics.

With --ranks N and --checkpoint FILE (DESIGN.md §3 rule 17) every rank writes its shard of the state
to FILE.g<generation>.r<rank>, and FILE itself becomes a small manifest naming them; --resume reads
the manifest and all its rank files and continues on any number of ranks, the saved number or
another (no --ranks: one), and a one-rank FILE resumes on several ranks as well.  A resume that
finds a rank file missing, or of another save than the manifest's, refuses.
"""
import argparse
import json
import logging
import os
import sys


MAX_RANKS = 16


def polls_from(paths, poll_bytes, first=0, offset=0):
    """polls() from byte `offset` of file `first` on, each piece with the position behind it:
    (text, file index, byte offset) of the next poll."""
    for k in range(first, len(paths)):
        with open(paths[k], "rb") as f:
            data = f.read()
        at = offset if k == first else 0
        while at < len(data):
            end = len(data) if len(data) - at <= poll_bytes else data.find(b"\n", at + poll_bytes - 1) + 1
            end = end if end > 0 else len(data)
            yield (data[at:end],) + ((k, end) if end < len(data) else (k + 1, 0))
            at = end


def polls(paths, poll_bytes):
    """The files' bytes in order, cut behind line ends into pieces of about poll_bytes."""
    for text, _, _ in polls_from(paths, poll_bytes):
        yield text


def write_checkpoint(path, blob):
    """Replace `path` by `blob` so that a reader sees the old file or the new one, never a part."""
    tmp = "%s.tmp.%d" % (path, os.getpid())
    with open(tmp, "wb") as f:
        f.write(blob)
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, path)


def rank_file(path, generation, rank):
    """The file of one rank's shard of a several-rank checkpoint (DESIGN.md §3 rule 17)."""
    return "%s.g%d.r%d" % (path, generation, rank)


def manifest_blob(user):
    """A snapshot blob (snapshot.hpp, version 1) that holds user bytes and nothing else: the manifest
    of a several-rank checkpoint.  engine.snapshot_info reads it like any other."""
    import struct
    seed, mask = 0x9E3779B97F4A7C15, (1 << 64) - 1

    def checksum(data):
        data = data + b"\0" * (-len(data) % 8)
        words = struct.unpack("<%dQ" % (len(data) // 8), data)
        return sum(((w ^ seed) * (2 * i + 1)) & mask for i, w in enumerate(words)) & mask
    user = bytes(user)
    total = 80 + ((len(user) + 15) & ~15)   # header 32, one table entry 40, padded to 80
    entry = struct.pack("<IIQQQQ", 1, 1, 80, len(user), len(user), checksum(user))
    tsum = checksum(struct.pack("<QIIQQ", 0x0150414E534D5253, 1, 1, total, 0) + entry)
    head = struct.pack("<QIIQQ", 0x0150414E534D5253, 1, 1, total, tsum) + entry
    return head + b"\0" * 8 + user + b"\0" * (-len(user) % 16)


def read_checkpoint(path):
    """The blobs a resume loads and their user records: FILE itself (a one-rank checkpoint), or, when
    FILE is the manifest of a several-rank one, every rank file of its generation -- all present and
    of that one save, else ValueError.  Returns (blobs, users, manifest or None)."""
    from . import engine
    with open(path, "rb") as f:
        blob = f.read()
    info = engine.snapshot_info(blob)
    user = json.loads(info["user"].decode())
    if "ranks" not in user:
        return [blob], [user], None
    blobs, users = [], []
    for r in range(user["ranks"]):
        p = rank_file(path, user["generation"], r)
        if not os.path.exists(p):
            raise ValueError("the checkpoint is incomplete: %s, which its manifest names, is missing" % p)
        with open(p, "rb") as f:
            blobs.append(f.read())
        u = json.loads(engine.snapshot_info(blobs[-1])["user"].decode())
        if u.get("generation") != user["generation"] or u.get("ranks") != user["ranks"] or u.get("rank") != r:
            raise ValueError("the checkpoint is incomplete: %s is of another save than its manifest" % p)
        users.append(u)
    return blobs, users, user


def write_flush(files, dest, k):
    from .batch import write_tiles
    out = {}
    for name, body in files.items():
        if os.path.exists(os.path.join(dest, name)):
            name = "%s.%d" % (name, k)
        out[name] = body.decode()
    write_tiles(out, dest)
    return len(out)


def run(paths, conf, dest, formatter, mode="auto", report_levels=(0, 1), transition_levels=(0, 1), privacy=2,
        quantisation=3600, flush_interval=300, source="smpl_rprt", max_vehicles=1 << 16, poll_bytes=1 << 20, device=0,
        report_dist_m=None, report_count=None, report_time_s=None, checkpoint=None, stop_after_polls=None, resume=False,
        comm=None):
    """comm: a dist.Comm of the stream's ranks (None: one rank).  Every rank calls run() with the
    same arguments; the statistics returned are summed over the ranks."""
    from . import engine
    from .batch import options_from_config
    opts, graph = options_from_config(conf, mode)
    fmt = engine.MessageFormat.from_spec(formatter)
    eng = engine.Engine(graph, device)
    with open(conf) as f:
        radius = json.load(f).get("reporter_amd", {}).get("ball_radius")
    if radius is not None:
        eng.set_ball_radius(float(radius))
    bm = engine.BatchMatcher(eng)
    sess = engine.VehicleSessions(bm, max_vehicles, report_dist_m, report_count, report_time_s, opts=opts,
                                  report_levels=report_levels, transition_levels=transition_levels)
    vdir = engine.VehicleDirectory(max_vehicles, device)
    store = engine.TileStore(device, quantisation, privacy, source, mode)
    stats = dict(polls=0, messages=0, dropped=0, forwarded=0, flushes=0, files=0)
    rank, nranks = (comm.rank, comm.world_size) if comm is not None else (0, 1)
    shard = (rank, nranks) if comm is not None else None
    last_flush = now = None
    inputs = [[os.path.abspath(p), os.path.getsize(p)] for p in paths]
    pos = [0, 0]   # file index and byte offset of the next poll
    # a several-rank checkpoint (rule 17): the generation last written and the rank files it has;
    # sharded: this stream's state is saved as shards (several ranks, or one that resumed from shards)
    generation, old_files, sharded = 0, [], comm is not None
    try:
        if resume:
            blobs, users, manifest = read_checkpoint(checkpoint)
            if (manifest or users[0])["inputs"] != inputs:
                raise ValueError("the checkpoint was written for other inputs (their list or sizes differ)")
            if (manifest or users[0]).get("done"):   # written behind the final flush: nothing is left to do
                return (manifest or users[0])["stats"]
            user = users[0]
            for u in users[1:]:   # the ranks ran in lockstep: position and stream time are replicated
                if any(u[k] != user[k] for k in ("inputs", "file", "offset", "now", "last_flush")):
                    raise ValueError("the checkpoint's rank files disagree on the stream's position")
            if manifest is None and comm is None and "nranks" not in engine.snapshot_info(blobs[0]):
                engine.load_stream(blobs[0], sess, vdir, store)
            else:
                engine.load_stream_shards(blobs, sess, vdir, store, shard=(rank, nranks))
                sharded = True
            pos, now, last_flush, stats = [user["file"], user["offset"]], user["now"], user["last_flush"], dict(user["stats"])
            for k in ("forwarded", "files"):   # what the saved ranks did apart: their sum to rank 0
                stats[k] = sum(u["stats"][k] for u in users) if rank == 0 else 0
            if manifest is not None:
                generation = manifest["generation"]
                old_files = [rank_file(checkpoint, generation, r) for r in range(manifest["ranks"])]

        def save(done=False):
            nonlocal generation, old_files
            user = dict(inputs=inputs, file=pos[0], offset=pos[1], now=now, last_flush=last_flush, stats=stats, done=done)
            if not sharded:
                write_checkpoint(checkpoint, engine.save_stream(sess, vdir, store, json.dumps(user).encode()))
                return
            # every rank its file of a new generation; then, all written, the manifest replaces FILE;
            # only then do the files of the generation before go: a run killed anywhere leaves a
            # manifest whose rank files all exist and are of one save
            generation += 1
            user.update(rank=rank, ranks=nranks, generation=generation)
            blob = engine.save_stream_shard(sess, vdir, store, (rank, nranks), json.dumps(user).encode())
            write_checkpoint(rank_file(checkpoint, generation, rank), blob)
            if comm is not None:
                comm.barrier()
            if rank == 0:
                head = dict(ranks=nranks, generation=generation, inputs=inputs, done=done)
                if done:
                    head["stats"] = stats
                write_checkpoint(checkpoint, manifest_blob(json.dumps(head).encode()))
                for p in old_files:
                    if os.path.exists(p):
                        os.remove(p)
            old_files = [rank_file(checkpoint, generation, r) for r in range(nranks)]

        def flush():
            if comm is not None:
                store.exchange(comm)   # every tile row to the rank that writes its file
            files, _ = store.flush()
            stats["files"] += write_flush(files, dest, stats["flushes"])
            stats["flushes"] += 1

        polled = 0
        for text, pos[0], pos[1] in polls_from(paths, poll_bytes, pos[0], pos[1]):
            out, info = sess.push_messages([text], fmt, vdir, shard=shard)
            store.add_session(sess)
            stats["polls"] += 1
            stats["messages"] += info["points"]
            stats["dropped"] += info["dropped"]
            stats["forwarded"] += out["forwarded"]
            for c, ln, why in sess.dropped_messages() if rank == 0 else ():
                logging.warning("poll %d line %d dropped: %s", stats["polls"], ln, why)
            span = sess.messages_span()
            if span is not None:
                now = span[1] if now is None else max(now, span[1])
                last_flush = span[0] if last_flush is None else last_flush
                if now - last_flush >= flush_interval:
                    flush()
                    last_flush = now
                    if checkpoint:
                        save()
            polled += 1
            if stop_after_polls is not None and polled >= stop_after_polls:
                break
        else:
            stop_after_polls = None   # the input ended first: finish as ever
        if stop_after_polls is not None:
            save()
            stats["stopped"] = True
            if comm is not None:
                for k in ("forwarded", "files"):
                    stats[k] = int(comm.allreduce_host(stats[k]))
            return stats
        if now is not None:
            out = sess.punctuate(int(now * 1000) + 10 ** 7)   # every vehicle is stale: all report and leave
            store.add_session(sess)
            stats["forwarded"] += out["forwarded"]
        flush()
        stats["vehicles"] = vdir.size
        if comm is not None:   # what the ranks did apart: summed (counts below 2^53 are exact in a double)
            for k in ("forwarded", "files"):
                stats[k] = int(comm.allreduce_host(stats[k]))
        if checkpoint:
            save(done=True)
        return stats
    finally:
        store.close()
        vdir.close()
        sess.close()
        bm.close()
        eng.close()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("inputs", nargs="+", help="files (or directories of files) of raw messages, one per line")
    ap.add_argument("--formatter", required=True, help="the reference's formatter string, e.g. ',sv,\\|,1,9,10,0,5' or "
                    "'@json@id@latitude@longitude@timestamp@accuracy'; a last argument is the date pattern of the "
                    "time, e.g. '@json@id@lat@lon@time@acc@yyyy-MM-dd'T'HH:mm:ssZZ' (DESIGN.md rule 18)")
    ap.add_argument("--match-config", required=True)
    ap.add_argument("--output-location", required=True, help="a directory for the tile files")
    ap.add_argument("--mode", default="auto")
    ap.add_argument("--reports", default="0,1")
    ap.add_argument("--transitions", default="0,1")
    ap.add_argument("--privacy", type=int, default=2)
    ap.add_argument("--quantisation", type=int, default=3600)
    ap.add_argument("--flush-interval", type=int, default=300)
    ap.add_argument("--source", default="smpl_rprt")
    ap.add_argument("--max-vehicles", type=int, default=1 << 16)
    ap.add_argument("--poll-bytes", type=int, default=1 << 20, help="about how much text goes into one push")
    ap.add_argument("--report-dist", type=float, help="session trigger distance in metres (default 500)")
    ap.add_argument("--report-count", type=int, help="session trigger point count (default 10)")
    ap.add_argument("--report-time", type=float, help="session trigger time in seconds (default 60)")
    ap.add_argument("--checkpoint", help="a file for the stream's state, written after every tile flush and at a stop")
    ap.add_argument("--stop-after-polls", type=int, help="stop after this many polls, without the final punctuate and "
                    "flush, leaving the checkpoint to --resume from")
    ap.add_argument("--resume", action="store_true", help="continue from --checkpoint")
    ap.add_argument("--ranks", type=int, default=1, help="run the stream on this many GPUs (at most %d), one process each" % MAX_RANKS)
    ap.add_argument("--transport", choices=("rccl", "host"), default="rccl", help="the ranks' exchange: RCCL, or gloo over "
                    "the host, with which several ranks can share one GPU")
    a = ap.parse_args(argv)
    if (a.resume or a.stop_after_polls is not None) and not a.checkpoint:
        ap.error("--resume and --stop-after-polls need --checkpoint")
    if not 1 <= a.ranks <= MAX_RANKS:
        ap.error("--ranks must be 1 .. %d" % MAX_RANKS)
    world = int(os.environ.get("WORLD_SIZE", "1")) if "RANK" in os.environ else 0
    if world and a.ranks > 1 and a.ranks != world:
        ap.error("--ranks %d under a launcher that started %d ranks (WORLD_SIZE)" % (a.ranks, world))
    if world > MAX_RANKS:
        ap.error("at most %d ranks" % MAX_RANKS)
    if a.ranks > 1 and not world:
        # this process has not opened the GPU and never does: each rank is a fresh child
        from .dist import self_launch
        return self_launch("reporter_amd.stream", sys.argv[1:] if argv is None else argv, a.ranks)
    paths = []
    for p in a.inputs:
        if os.path.isdir(p):
            for root, _, fs in sorted(os.walk(p)):
                paths += [os.path.join(root, f) for f in sorted(fs)]
        else:
            paths.append(p)
    levels = lambda s: tuple(int(x) for x in s.split(",") if x != "")
    device = int(os.environ.get("LOCAL_RANK", "0"))
    comm = None
    if world > 1:
        import ctypes
        from . import _lib, dist
        cnt = ctypes.c_int(0)
        _lib.check(_lib.lib().rm_device_count(ctypes.byref(cnt)))
        if a.transport == "rccl" and world > cnt.value:
            ap.error("--transport rccl needs a GPU per rank (%d ranks, %d devices): use --transport host" % (world, cnt.value))
        device %= max(cnt.value, 1)
        comm = dist.stream_comm(int(os.environ["RANK"]), world, device, a.transport)
    stats = run(paths, a.match_config, a.output_location, a.formatter, a.mode, levels(a.reports), levels(a.transitions),
                a.privacy, a.quantisation, a.flush_interval, a.source, a.max_vehicles, a.poll_bytes,
                device, a.report_dist, a.report_count, a.report_time, a.checkpoint,
                a.stop_after_polls, a.resume, comm)
    if comm is not None:
        comm.close()   # (a rank that failed above leaves without the closing barrier: the launcher ends the others)
    if comm is None or comm.rank == 0:
        print(json.dumps(stats))
    return 0


if __name__ == "__main__":
    sys.exit(main())
