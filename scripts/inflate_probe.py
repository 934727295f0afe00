"""Gzip ingest probe (rule 20): from a directory of .gz trace files to parsed points,
the device inflate against two baselines that are not the code under test.

    python scripts/inflate_probe.py [--vehicles 10000] [--points 600] [--files 16,256,1024,4096]
                                    [--repeats 5] [--out profiles/inflate/inflate_probe.json]

The C2-shaped workload of scripts/lines_probe.py (vehicles x points lines, shuffled) is split evenly
by lines into F files, each gzip level 6 from Python's zlib.  Per F, `repeats` calls after a warm-up,
every figure as (min, max):
  device route   RM_INFLATE_DEVICE_MIN_CHUNKS=0: upload of the compressed bytes, inflate (with the
                 CRC), gather, parse (BatchMatcher.lines_ms / inflate_ms), and the call's wall time;
  host route     the same decoder core on the host pool, then the plain upload: the call's wall time;
  plain          the same text uncompressed through parse_lines: upload, parse, wall time;
  zlib-16        zlib's own inflate on 16 host threads over the same files
                 (scripts/cpp/zlib_inflate_bench.cpp).
The device route is ahead at an F where upload(gz) + inflate + crc + gather is below zlib-16 +
upload(plain) by more than the repeats' spread.  The single large file: the largest file of the
F = 16 split alone, one wave against one zlib thread.  Prints one JSON line and writes it to --out."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from reporter_amd import _lib, engine, world   # noqa: E402

BENCH = os.path.join(ROOT, "scripts", "bin", "zlib_inflate_bench")


def build_bench():
    src = os.path.join(ROOT, "scripts", "cpp", "zlib_inflate_bench.cpp")
    if os.path.exists(BENCH) and os.path.getmtime(BENCH) >= os.path.getmtime(src):
        return
    os.makedirs(os.path.dirname(BENCH), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", src, "-o", BENCH, "-lz", "-lpthread"], check=True)


def gz(data):
    z = zlib.compressobj(6, zlib.DEFLATED, 31)
    return z.compress(data) + z.flush()


def span(xs):
    return [round(min(xs), 3), round(max(xs), 3)]


def parse(bm, chunks, coding, min_chunks, repeats):
    """repeats calls of rm_runner_parse_lines after one warm-up: the parts' (min, max) in ms"""
    os.environ["RM_INFLATE_DEVICE_MIN_CHUNKS"] = str(min_chunks)
    bm.set_input_coding(coding)
    d, keep = engine._lines_desc(chunks, None, 120.0, None)
    rows = []
    for r in range(repeats + 1):
        t0 = time.perf_counter()
        _lib.check(_lib.lib().rm_runner_parse_lines(bm._h, C.byref(d)))
        wall = (time.perf_counter() - t0) * 1e3
        if r:
            rows.append(dict(bm.lines_ms(), **bm.inflate_ms(), wall=wall))
    out = {k: span([row[k] for row in rows]) for k in ("upload", "inflate", "crc", "gather", "parse", "ids", "wall")}
    out["info"] = bm.inflate_info()
    out["lines"] = bm.lines_info()["lines"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vehicles", type=int, default=10000)
    ap.add_argument("--points", type=int, default=600)
    ap.add_argument("--rows", type=int, default=80)
    ap.add_argument("--files", default="16,256,1024,4096")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "inflate", "inflate_probe.json"))
    a = ap.parse_args()
    build_bench()
    tmp = tempfile.mkdtemp(prefix="inflate_probe")
    graph = os.path.join(tmp, "g.rmg")
    world.build_world(graph, a.rows, a.rows, 100.0, seed=1)
    tr = world.generate_traces(graph, n_traces=a.vehicles, n_points=a.points, rate_s=1.0, noise_m=5.0, seed=5)
    n = a.vehicles * a.points
    veh = np.repeat(np.arange(a.vehicles), a.points)
    perm = np.random.default_rng(1).permutation(n)
    lat, lon, tm, acc = tr["lat"][perm], tr["lon"][perm], tr["time"][perm].astype(np.int64), tr["accuracy"][perm]
    lines = []
    step = 1 << 20
    for s in range(0, n, step):
        e = min(n, s + step)
        lines += ["veh-%08x,%d,%.6f,%.6f,%d\n" % r for r in zip(veh[perm[s:e]].tolist(), tm[s:e].tolist(), lat[s:e].tolist(),
                                                               lon[s:e].tolist(), acc[s:e].astype(np.int64).tolist())]
    eng = engine.Engine(graph, 0)
    bm = engine.BatchMatcher(eng)
    out = dict(vehicles=a.vehicles, points_per_vehicle=a.points, lines=n, level=6, zlib=zlib.ZLIB_RUNTIME_VERSION, repeats=a.repeats,
               by_files={})
    single = None
    for F in [int(x) for x in a.files.split(",")]:
        plain = ["".join(lines[n * k // F:n * (k + 1) // F]).encode() for k in range(F)]
        with ThreadPoolExecutor(16) as ex:
            packed = list(ex.map(gz, plain))
        d = os.path.join(tmp, "f%d" % F)
        os.makedirs(d)
        for k, z in enumerate(packed):
            with open(os.path.join(d, "%05d.gz" % k), "wb") as f:
                f.write(z)
        row = dict(files=F, bytes_plain=sum(len(c) for c in plain), bytes_gz=sum(len(z) for z in packed))
        row["device"] = parse(bm, packed, "gzip", 0, a.repeats)
        row["host_route"] = parse(bm, packed, "gzip", 1 << 30, a.repeats)
        row["plain"] = parse(bm, plain, "plain", 0, a.repeats)
        r = subprocess.run([BENCH, d, "16", str(a.repeats)], capture_output=True, text=True, check=True)
        row["zlib16_ms"] = span(json.loads(r.stdout)["ms"])
        dev = [row["device"][k] for k in ("upload", "inflate", "crc", "gather")]
        row["device_sum_ms"] = [round(sum(x[0] for x in dev), 3), round(sum(x[1] for x in dev), 3)]
        row["baseline_sum_ms"] = [round(row["zlib16_ms"][0] + row["plain"]["upload"][0], 3),
                                  round(row["zlib16_ms"][1] + row["plain"]["upload"][1], 3)]
        row["device_ahead"] = row["device_sum_ms"][1] < row["baseline_sum_ms"][0]
        out["by_files"][str(F)] = row
        print(json.dumps(row), flush=True)
        if single is None:   # the largest file of the first split alone: one wave against one zlib thread
            k = max(range(F), key=lambda i: len(packed[i]))
            one = os.path.join(tmp, "one")
            os.makedirs(one)
            with open(os.path.join(one, "0.gz"), "wb") as f:
                f.write(packed[k])
            r = subprocess.run([BENCH, one, "1", str(a.repeats)], capture_output=True, text=True, check=True)
            single = dict(bytes_plain=len(plain[k]), bytes_gz=len(packed[k]), zlib1_ms=span(json.loads(r.stdout)["ms"]),
                          device=parse(bm, [packed[k]], "gzip", 0, a.repeats))
            print(json.dumps(single), flush=True)
    out["single_file"] = single
    os.environ.pop("RM_INFLATE_DEVICE_MIN_CHUNKS", None)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    bm.close()
    eng.close()


if __name__ == "__main__":
    main()
