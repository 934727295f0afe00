"""Date pattern probe (DESIGN.md §3 rule 18): what reading the time by a compiled pattern costs in
the `parse` stage of VehicleSessions.push_messages, on scripts/stream_probe.py's workload.

    python scripts/time_pattern_probe.py [--vehicles 10000] [--per-push 60] [--runs 6] [--root DIR]
                                         [--out profiles/time_patterns/probe.json]

One push of C2's traces (10,000 vehicles x 60 points: 600 k messages) is written as separated
values and as JSON, the same instants in four spellings: epoch seconds (time_format 0),
yyyy-MM-dd HH:mm:ss (time_format 1), yyyy-MM-dd'T'HH:mm:ss.SSSZZ with a +08:00 offset and
dd/MMM/yyyy HH:mm:ss (patterns).  After a warm-up push of each, the eight texts are pushed in turn,
--runs times over, each into new sessions; reported per text: its bytes per message and the parse
stage's device ms of every run (rm_session_messages_time), with the text upload beside it.

--root names another tree whose reporter_amd is measured instead (the parent commit's, built, for
the comparison of time_format 0 and 1); a tree without rm_time_pattern measures those two alone."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MONTHS = ("Jan", "Feb", "Mar", "Apr", "May", "Jun", "Jul", "Aug", "Sep", "Oct", "Nov", "Dec")
ISO = "yyyy-MM-dd'T'HH:mm:ss.SSSZZ"
NAMED = "dd/MMM/yyyy HH:mm:ss"


def spell(t, how, j):
    if how == "epoch":
        return "%d" % t
    if how == "civil":
        return "%04d-%02d-%02d %02d:%02d:%02d" % time.gmtime(t)[:6]
    if how == "iso":
        return "%04d-%02d-%02dT%02d:%02d:%02d" % time.gmtime(t + 8 * 3600)[:6] + ".%03d+08:00" % (j % 1000)
    g = time.gmtime(t)
    return "%02d/%s/%04d %02d:%02d:%02d" % (g[2], MONTHS[g[1] - 1], g[0], g[3], g[4], g[5])


def write_text(arr, kind, how):
    rows = []
    quote = '"%s"' if how != "epoch" else "%s"
    for j, (v, t, la, lo, ac) in enumerate(zip(arr["vehicle"].tolist(), arr["time"].astype(np.int64).tolist(), arr["lat"].tolist(),
                                               arr["lon"].tolist(), arr["accuracy"].tolist())):
        tm = spell(t, how, j)
        if kind == 0:
            rows.append("veh-%07d,%s,%.6f,%.6f,%.1f" % (v, tm, la, lo, ac))
        else:
            rows.append('{"id":"veh-%07d","timestamp":%s,"latitude":%.6f,"longitude":%.6f,"accuracy":%.1f}' % (v, quote % tm, la, lo, ac))
    return ("\n".join(rows) + "\n").encode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vehicles", type=int, default=10000)
    ap.add_argument("--per-push", type=int, default=60)
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--out", default=os.path.join("profiles", "time_patterns", "probe.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    from reporter_amd import engine, world
    cfg = world.CONFIGS["C2"]
    tmp = tempfile.mkdtemp(prefix="time_pattern_probe")
    graph = os.path.join(tmp, "c2.rmg")
    world.build_world(graph, cfg["rows"], cfg["cols"], cfg["block_m"], seed=1, cell_m=cfg["cell_m"])
    T, n = a.vehicles, a.per_push
    tr = world.generate_traces(graph, n_traces=T, n_points=n, rate_s=cfg["rate_s"], noise_m=cfg["noise_m"], seed=1000)
    order = np.arange(T * n).reshape(T, n).T.ravel()   # time-major, as stream_probe.py writes it
    arr = {"vehicle": (order // n).astype(np.uint32)}
    for f in ("time", "lon", "lat", "accuracy"):
        arr[f] = np.ascontiguousarray(tr[f][order])
    patterns = hasattr(engine, "time_pattern_id")
    line = {"epoch": lambda: engine.LineFormat(), "civil": lambda: engine.LineFormat(time_format=1)}
    if patterns:
        line["iso"] = lambda: engine.LineFormat(time_pattern=ISO)
        line["named"] = lambda: engine.LineFormat(time_pattern=NAMED)
    cases = [(kind, how) for kind in (0, 1) for how in line]
    texts = {c: write_text(arr, *c) for c in cases}
    fmts = {(kind, how): engine.MessageFormat(kind, line[how]()) for kind, how in cases}
    print("texts written", file=sys.stderr, flush=True)
    eng = engine.Engine(graph, 0)
    bm = engine.BatchMatcher(eng)

    def push(c):
        sess = engine.VehicleSessions(bm, T)
        vdir = engine.VehicleDirectory(T)
        out, info = sess.push_messages([texts[c]], fmts[c], vdir)
        ms = sess.messages_ms()
        vdir.close()
        sess.close()
        assert info["points"] == T * n and info["host_lines"] == 0 and info["dropped"] == 0, info
        return ms

    for c in cases:
        push(c)
    runs = {c: [] for c in cases}
    for _ in range(a.runs):
        for c in cases:
            runs[c].append(push(c))
    rows = []
    for kind, how in cases:
        parse = [round(r["parse"], 4) for r in runs[(kind, how)]]
        rows.append(dict(kind="json" if kind else "sv", time=how, bytes_per_message=round(len(texts[(kind, how)]) / (T * n), 2),
                         parse_ms=parse, parse_ms_min=min(parse), parse_ms_median=float(np.median(parse)), parse_ms_max=max(parse),
                         text_upload_ms=[round(r["text_upload"], 4) for r in runs[(kind, how)]]))
    out = dict(args=dict(vehicles=T, per_push=n, runs=a.runs), messages_per_push=T * n, patterns=dict(iso=ISO, named=NAMED) if patterns else None,
               order="the texts in turn within a run, runs back to back in one process", rows=rows)
    text = json.dumps(out)
    print(text)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    bm.close()
    eng.close()


if __name__ == "__main__":
    main()
