"""Tile store probe (rule 13): synthetic segments through TileStore.add in calls of
--call segments, then one flush.

    python scripts/tilestore_probe.py [--segments 4000000] [--call 65536] [--tiles 1000] [--hours 24]
                                      [--privacy 2] [--out profiles/tilestore/tilestore_probe.json]

The segments spread over --tiles tile ids x --hours one-hour buckets; each tile id has 16 ids with
4 next ids each, so nearly every (id, next_id) range of a file passes the privacy count.  Recorded:
the six device parts of rm_tilestore_time summed over the adds and of the flush, rows and bytes,
the text stage's bytes/s beside the float4 copy rate bench.py divides by (frac_vs_measured_copy),
and the host time of formatting as many rows with an snprintf loop like rm_runner_tiles'
format_row (scripts/tile_format_host.cpp), the thing the device text replaces.  Prints one JSON
line and writes it to --out."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from reporter_amd import engine   # noqa: E402

PARTS = ("upload", "expand", "sort", "cull", "text", "download")
HBM_MEASURED_GBS = 6290.0   # bench.py: the float4 copy ceiling frac_vs_measured_copy divides by


def segments(n, tiles, hours, seed=7):
    rng = np.random.default_rng(seed)
    tile = (rng.integers(0, tiles, n).astype(np.uint64) << np.uint64(3)) | np.uint64(1)
    ident = tile | (rng.integers(1, 17, n).astype(np.uint64) << np.uint64(25))
    nxt = np.where(rng.integers(0, 4, n) == 0, np.uint64(engine.INVALID_SEGMENT_ID),
                   tile | (rng.integers(17, 20, n).astype(np.uint64) << np.uint64(25)))
    t0 = 1.5e9 + rng.integers(0, hours * 3600 - 400, n).astype(np.float64) + rng.integers(0, 4, n) / 4.0
    t1 = t0 + rng.integers(4, 1200, n) / 4.0
    return ident, nxt.astype(np.uint64), t0, t1, rng.integers(50, 2000, n).astype(np.int32), rng.integers(0, 100, n).astype(np.int32)


def host_baseline(cols, rows, q, source, mode, tmp):
    exe = os.path.join(tmp, "tile_format_host")
    subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "scripts", "tile_format_host.cpp"), "-o", exe], check=True)
    a = np.empty(len(cols[0]), engine.TILE_SEGMENT_DTYPE)
    for name, x in zip(engine.TILE_SEGMENT_DTYPE.names, cols):
        a[name] = x
    path = os.path.join(tmp, "segments.bin")
    a.tofile(path)
    r = subprocess.run([exe, path, str(rows), str(q), source, mode.upper()], check=True, capture_output=True, text=True, timeout=600)
    return json.loads(r.stdout)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=4000000)
    ap.add_argument("--call", type=int, default=65536)
    ap.add_argument("--tiles", type=int, default=1000)
    ap.add_argument("--hours", type=int, default=24)
    ap.add_argument("--privacy", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "tilestore", "tilestore_probe.json"))
    a = ap.parse_args()
    q, source, mode = 3600, "smpl_rprt", "auto"
    cols = segments(a.segments, a.tiles, a.hours)
    runs = []
    for run in range(2):   # the first run grows the buffers; the second is the steady one
        store = engine.TileStore(0, q, a.privacy, source, mode) if run == 0 else store
        add_ms = dict.fromkeys(PARTS, 0.0)
        t_add = time.perf_counter()
        held = 0
        for s in range(0, a.segments, a.call):
            c = store.add(*[x[s:s + a.call] for x in cols])
            held = c["held"]
            for k, v in store.ms().items():
                add_ms[k] += v
        add_wall = time.perf_counter() - t_add
        t0 = time.perf_counter()
        files, counts = store.flush()
        flush_wall = time.perf_counter() - t0
        ms = store.ms()
        dev_ms = sum(ms[p] for p in ("sort", "cull", "text"))
        text_gbs = counts["bytes"] / (ms["text"] * 1e-3) / 1e9 if ms["text"] else None
        runs.append(dict(add_calls=(a.segments + a.call - 1) // a.call, add_wall_s=add_wall, add_ms={k: round(v, 3) for k, v in add_ms.items()},
                         add_segments_per_s=a.segments / add_wall, rows_held=held, flush_wall_s=flush_wall,
                         flush_ms={k: round(v, 3) for k, v in ms.items()}, counts=counts,
                         flush_rows_per_s_device=counts["rows_in"] / (dev_ms * 1e-3), flush_rows_per_s_wall=counts["rows_in"] / flush_wall,
                         text_gbs=text_gbs, text_frac_vs_measured_copy=text_gbs / HBM_MEASURED_GBS if text_gbs else None,
                         bytes_per_kept_row=counts["bytes"] / max(counts["rows_kept"], 1)))
        del files
    store.close()
    with tempfile.TemporaryDirectory() as tmp:
        host = host_baseline(cols, runs[-1]["counts"]["rows_kept"], q, source, mode, tmp)
    out = dict(segments=a.segments, call=a.call, tiles=a.tiles, hours=a.hours, privacy=a.privacy, quantisation=q,
               copy_rate_gbs=HBM_MEASURED_GBS, runs=runs, host_snprintf=host,
               host_ms_over_device_text_ms=host["ms"] / runs[-1]["flush_ms"]["text"] if runs[-1]["flush_ms"]["text"] else None)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
