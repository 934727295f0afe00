"""GPU batch reporter: the match and report phases of reference py/simple_reporter.py
on local files, with every stage on the MI355X.

    python -m reporter_amd.batch --trace-dir traces/ --match-config conf.json --dest-dir out/
    python -m torch.distributed.run --nproc-per-node 8 -m reporter_amd.batch ...   (one rank per GPU)

Input: the trace files simple_reporter's download phase writes (one point per line,
``uuid,time,lat,lon,accuracy``, py/simple_reporter.py:113; files named by a uuid hash,
:116).  Output: one file per time tile at ``<dest>/<start>_<end>/<level>/<tile index>``
holding exactly the text the reference's report phase would upload for that tile
(header + privacy-culled rows in string order, :211-254).

Reference phases and what replaces them:
  match()   :131-209  group by uuid, sort, inactivity windows      -> rm_runner_run_points
                      Match + report() per window                   -> the matcher kernels + k_report
                      valid-report filter, hour buckets, rows       -> rm_runner_tiles (rows)
  report()  :211-254  sort, privacy cull, CSV, upload               -> rm_runner_tiles (cull + CSV)
Ingest: the files' lines are parsed and the vehicle ids numbered on the GPU as well
(--ingest device, the default: rm_runner_run_lines); --ingest host keeps the interpreted loop
(read_trace_files + dense_ids) in front of rm_runner_run_points.  --formatter takes one of the
reference's separated-value formatter strings (Formatter.java:36-51), --bbox and --accuracy-cap
the download phase's filter and cap (py/simple_reporter.py:105,112), so raw lines can be read too.
--input gzip (or auto: by the magic bytes 1f 8b) reads the reference's own source files, which are
gzip (load_data.sh:11, py/simple_reporter.py:99): they are inflated and checked on the GPU
(DESIGN.md rule 20); a file that does not inflate is logged and skipped (:128-129).
Multi-GPU: trace files are block-split over ranks (simple_reporter.split, :70-79, the
reference's process split); rows of every rank are all-gathered over RCCL and each rank
writes the tile files it owns.  There is no CPU path: the library raises without a GPU.
"""
import argparse
import json
import logging
import os
import sys

import numpy as np


def read_trace_files(paths):
    """Points of simple_reporter trace files -> (uuid strings, arrays).  Lines are
    ``uuid,time,lat,lon,accuracy`` (:113, parsed as :139-140: int time, float lat/lon,
    int accuracy)."""
    uuids, tm, lat, lon, acc = [], [], [], [], []
    for p in paths:
        with open(p, "r") as f:
            for line in f:
                line = line.strip()
                if not line:
                    continue
                u, t, la, lo, a = line.split(",")
                uuids.append(u)
                tm.append(int(t))
                lat.append(float(la))
                lon.append(float(lo))
                acc.append(int(a))
    return uuids, dict(time=np.asarray(tm, np.float64), lat=np.asarray(lat, np.float64),
                       lon=np.asarray(lon, np.float64), accuracy=np.asarray(acc, np.float32))


def dense_ids(uuids):
    """Dense vehicle index per point, in first-seen order; returns (index array, names)."""
    table = {}
    idx = np.empty(len(uuids), np.uint32)
    for k, u in enumerate(uuids):
        idx[k] = table.setdefault(u, len(table))
    return idx, list(table)


def options_from_config(conf_path, mode):
    """meili defaults (+ the mode's section) of a Valhalla-style config, as rm_configure reads it."""
    from . import engine
    from .world import MODES
    o = engine.default_options(1, mode=MODES[mode])
    with open(conf_path) as f:
        conf = json.load(f)
    meili = conf.get("meili", {})
    for section in (meili.get("default", {}), meili.get(mode, {})):
        for k, v in section.items():
            if k in o.dtype.names and k != "mode":
                o[k] = v
    graph = conf.get("reporter_amd", {}).get("graph") or conf.get("mjolnir", {}).get("tile_extract")
    if not graph:
        raise ValueError("config names no graph (reporter_amd.graph or mjolnir.tile_extract)")
    if not os.path.isabs(graph):
        graph = os.path.join(os.path.dirname(os.path.abspath(conf_path)), graph)
    return o, graph


def write_tiles(files, dest_dir):
    """{tile name: text} -> files under dest_dir (one file per tile, as uploaded)."""
    for name, body in files.items():
        path = os.path.join(dest_dir, name)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(body)


def read_chunks(paths):
    """The files' bytes, one chunk per file (mapped, not copied, where the file is not empty)."""
    import mmap
    chunks = []
    for p in paths:
        with open(p, "rb") as f:
            chunks.append(mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) if os.fstat(f.fileno()).st_size else b"")
    return chunks


def run(trace_files, conf, dest_dir, mode="auto", report_levels=(0, 1), transition_levels=(0, 1), quantisation=3600,
        inactivity=120, privacy=2, source="smpl_rprt", rank=0, world=1, device=0, comm=None, ingest="device", fmt=None,
        bbox=None, coding="plain"):
    from . import dist, engine
    if ingest not in ("device", "host"):
        raise ValueError("ingest is 'device' or 'host'")
    if coding not in engine.INPUT_CODINGS:
        raise ValueError("coding is 'plain', 'gzip' or 'auto'")
    if coding != "plain" and ingest != "device":
        raise ValueError("gzip input needs ingest='device'")
    mine = dist.split(sorted(trace_files), world)[rank] if world > 1 else sorted(trace_files)
    opts, graph = options_from_config(conf, mode)
    if ingest == "host":
        if fmt is not None or bbox is not None:
            raise ValueError("a line format or box needs ingest='device'")
        uuids, pts = read_trace_files(mine)
        idx, names = dense_ids(uuids)
    else:
        chunks = read_chunks(mine)
        fmt = fmt or engine.LineFormat()
        if bbox is not None:
            fmt.bbox = tuple(float(x) for x in bbox)
    eng = engine.Engine(graph, device)
    with open(conf) as f:
        radius = json.load(f).get("reporter_amd", {}).get("ball_radius")
    if radius is not None:
        eng.set_ball_radius(float(radius))
    bm = engine.BatchMatcher(eng)
    bm.set_isolation(True)   # a failing window is logged and skipped (py/simple_reporter.py:169-173)
    try:
        if ingest == "host":
            bm.run_points(idx, pts["time"], pts["lon"], pts["lat"], pts["accuracy"], inactivity=inactivity, opts=opts,
                          n_uuids=len(names), report_levels=report_levels, transition_levels=transition_levels)
        else:
            bm.set_input_coding(coding, skip_bad=True)
            bm.run_lines(chunks, fmt, inactivity=inactivity, opts=opts, report_levels=report_levels,
                         transition_levels=transition_levels)
            for path, status in zip(mine, bm.chunk_status()):
                if status:
                    logging.error("%s was not processed: %s", path, engine.inflate_status_text(status))
        errs = bm.trace_errors()
        if errs.any():
            owner = bm.trace_uuid()
            if ingest == "device":
                names = bm.vehicle_names(chunks if coding == "plain" else None)
            for k in np.nonzero(errs)[0]:
                logging.error("%s window %d failed to match (error bits %d); skipped", names[owner[k]], k, int(errs[k]))
        files = bm.tiles(quantisation=quantisation, privacy=privacy, source=source, mode=mode, comm=comm)
        write_tiles(files, dest_dir)
        return files
    finally:
        bm.close()
        eng.close()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--trace-dir", required=True, help="directory of parsed trace files (simple_reporter --trace-dir)")
    ap.add_argument("--match-config", required=True)
    ap.add_argument("--dest-dir", required=True)
    ap.add_argument("--mode", default="auto")
    ap.add_argument("--report-levels", default="0,1")
    ap.add_argument("--transition-levels", default="0,1")
    ap.add_argument("--quantisation", type=int, default=3600)
    ap.add_argument("--inactivity", type=int, default=120)
    ap.add_argument("--privacy", type=int, default=2)
    ap.add_argument("--source-id", default="smpl_rprt")
    ap.add_argument("--ingest", choices=("device", "host"), default="device", help="where the trace lines are parsed")
    ap.add_argument("--input", choices=("plain", "gzip", "auto"), default="plain", help="the files' coding: gzip files are "
                    "inflated on the GPU (auto: those that begin 1f 8b); needs --ingest device")
    ap.add_argument("--formatter", help="separated-value formatter string, e.g. ',sv,\\|,1,9,10,0,5,yyyy-MM-dd HH:mm:ss' "
                    "(default: the trace files' uuid,time,lat,lon,accuracy); the last argument is a date pattern, "
                    "e.g. yyyy-MM-dd'T'HH:mm:ssZZ or yyyyMMddHHmmss (DESIGN.md rule 18)")
    ap.add_argument("--bbox", help="min_lat,min_lon,max_lat,max_lon: points outside are dropped")
    ap.add_argument("--accuracy-cap", type=int, default=0, help="cap on the accuracy column (0: none)")
    a = ap.parse_args(argv)
    files = []
    for root, _, fs in os.walk(a.trace_dir):
        files += [os.path.join(root, f) for f in fs]
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    comm = None
    if world > 1:
        from . import dist
        comm = dist.Comm(rank, world, local)
    levels = lambda s: tuple(int(x) for x in s.split(",") if x != "")
    fmt = None
    if a.formatter or a.accuracy_cap:
        from . import engine
        fmt = engine.LineFormat.from_spec(a.formatter) if a.formatter else engine.LineFormat()
        fmt.accuracy_cap = a.accuracy_cap
    bbox = [float(x) for x in a.bbox.split(",")] if a.bbox else None
    if bbox is not None and len(bbox) != 4:
        ap.error("--bbox takes min_lat,min_lon,max_lat,max_lon")
    if a.input != "plain" and a.ingest != "device":
        ap.error("--input gzip and auto need --ingest device")
    try:
        out = run(files, a.match_config, a.dest_dir, a.mode, levels(a.report_levels), levels(a.transition_levels),
                  a.quantisation, a.inactivity, a.privacy, a.source_id, rank, world, local, comm, a.ingest, fmt, bbox, a.input)
    finally:
        if comm is not None:
            comm.close()
    print(json.dumps({"rank": rank, "tiles": len(out), "rows": sum(b.count("\n") - 1 for b in out.values())}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
