"""Ingest probe: the time from trace-file text to the start of matching, today's interpreted path
against the device line reader (rule 11).

    python scripts/lines_probe.py [--vehicles 10000] [--points 600] [--out profiles/lines/lines_probe.json]

Writes one C2-shaped trace file (vehicles x points lines ``uuid,time,lat,lon,accuracy``, shuffled;
10,000 x 600 is about 250 MB) and times
  host path:   read_trace_files + dense_ids (the interpreted loop), then run_points' upload and
               window stage, taken as a run over the points less the same batch's rerun;
  device path: run_lines' upload, parse, ids and windows parts (BatchMatcher.lines_ms()).
Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from reporter_amd import batch, engine, world   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vehicles", type=int, default=10000)
    ap.add_argument("--points", type=int, default=600)
    ap.add_argument("--rows", type=int, default=80)
    ap.add_argument("--host-fraction", type=float, default=1.0, help="part of the file the interpreted loop reads (scaled up)")
    ap.add_argument("--skip-host", action="store_true", help="time the device path only (kernel traces)")
    ap.add_argument("--calls", type=int, default=3, help="run_lines calls; the last one is reported")
    ap.add_argument("--out", default=os.path.join("profiles", "lines", "lines_probe.json"))
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="lines_probe")
    graph = os.path.join(tmp, "g.rmg")
    world.build_world(graph, a.rows, a.rows, 100.0, seed=1)
    tr = world.generate_traces(graph, n_traces=a.vehicles, n_points=a.points, rate_s=1.0, noise_m=5.0, seed=5)
    n = a.vehicles * a.points
    veh = np.repeat(np.arange(a.vehicles), a.points)
    perm = np.random.default_rng(1).permutation(n)
    t0 = time.perf_counter()
    # vectorised formatting of n lines (np.char is slow but not what is measured)
    lat, lon, tm, acc = tr["lat"][perm], tr["lon"][perm], tr["time"][perm].astype(np.int64), tr["accuracy"][perm]
    path = os.path.join(tmp, "000")
    with open(path, "w") as f:
        step = 1 << 20
        for s in range(0, n, step):
            e = min(n, s + step)
            f.write("".join("veh-%08x,%d,%.6f,%.6f,%d\n" % r for r in zip(veh[perm[s:e]].tolist(), tm[s:e].tolist(),
                                                                       lat[s:e].tolist(), lon[s:e].tolist(),
                                                                       acc[s:e].astype(np.int64).tolist())))
    write_s = time.perf_counter() - t0
    size = os.path.getsize(path)
    eng = engine.Engine(graph, 0)
    bm = engine.BatchMatcher(eng)
    # ---- device path (the first call allocates; the last is reported)
    chunks = batch.read_chunks([path])
    dev = []
    for _ in range(max(a.calls, 1)):
        t0 = time.perf_counter()
        bm.run_lines(chunks, inactivity=120)
        wall = time.perf_counter() - t0
        t1 = time.perf_counter()
        bm.rerun()
        rerun = time.perf_counter() - t1
        ms = bm.lines_ms()
        dev.append(dict(ms, wall_to_match_ms=(wall - rerun) * 1e3, info=bm.lines_info(), traces=bm.sizes()["traces"]))
    # ---- today's path
    host = None
    if not a.skip_host:
        t0 = time.perf_counter()
        if a.host_fraction < 1.0:   # a prefix of the file, scaled: the loop is linear in the lines
            part = os.path.join(tmp, "part")
            with open(path, "rb") as f, open(part, "wb") as g:
                blob = f.read(int(size * a.host_fraction))
                g.write(blob[: blob.rfind(b"\n") + 1])
            t0 = time.perf_counter()
            uuids, pts = batch.read_trace_files([part])
        else:
            uuids, pts = batch.read_trace_files([path])
        read_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        idx, names = batch.dense_ids(uuids)
        ids_s = time.perf_counter() - t0
        scale = n / len(uuids)
        t0 = time.perf_counter()
        bm.run_points(idx, pts["time"], pts["lon"], pts["lat"], pts["accuracy"], inactivity=120, n_uuids=len(names))
        run_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        bm.rerun()
        rerun_s = time.perf_counter() - t0
        host = dict(read_trace_files_ms=read_s * 1e3 * scale, dense_ids_ms=ids_s * 1e3 * scale,
                    run_points_to_match_ms=(run_s - rerun_s) * 1e3 * scale, lines_read=len(uuids), scaled_by=scale)
        host["total_ms"] = host["read_trace_files_ms"] + host["dense_ids_ms"] + host["run_points_to_match_ms"]
    d = dev[-1]
    d["total_ms"] = d["upload"] + d["parse"] + d["ids"] + d["windows"]
    out = dict(vehicles=a.vehicles, points_per_vehicle=a.points, lines=n, bytes=size, write_file_s=write_s, host_path=host,
               device_path=d, device_first_call=dev[0], parse_gb_per_s=size / (d["parse"] * 1e-3) / 1e9 if d["parse"] else None,
               speedup=host["total_ms"] / d["total_ms"] if host and d["total_ms"] else None)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    bm.close()
    eng.close()


if __name__ == "__main__":
    main()
