"""Vehicle sessions probe (rule 12): C2's workload as a stream through
VehicleSessions, beside the same points through run_points in one call.

    python scripts/session_probe.py [--vehicles 10000] [--points 600] [--slice 10] [--runs 2]
                                    [--out profiles/sessions/session_probe.json]

The vehicles' traces are replayed in time order in slices of --slice seconds (10,000 x 600 at 1 Hz
in 10 s slices: 60 pushes of 100 k arrivals), then one punctuate evicts what is left.  Per push:
wall ms, the five device parts of rm_session_time and the counts; overall points/s.  The stream and
the one-call run_points alternate --runs times in one process.  Prints one JSON line and writes it
to --out."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from reporter_amd import engine, world   # noqa: E402

PARTS = ("upload", "append", "trigger", "match", "trim")


def stream(bm, arr, cuts, n_vehicles):
    sess = engine.VehicleSessions(bm, n_vehicles)
    pushes, total = [], dict.fromkeys(engine.SESSION_COUNTS, 0)
    t_all = time.perf_counter()
    matched = 0
    for a, b in cuts:
        t0 = time.perf_counter()
        out = sess.push(arr["vehicle"][a:b], arr["time"][a:b], arr["lon"][a:b], arr["lat"][a:b], arr["accuracy"][a:b],
                        arr["stamp_ms"][a:b])
        wall = (time.perf_counter() - t0) * 1e3
        ms = sess.ms()
        matched += int(sess.windows()["n_points"].sum())   # (outside the push's wall time)
        pushes.append([round(wall, 3)] + [round(ms[p], 3) for p in PARTS] + [out["triggers"], out["rounds"], out["forwarded"]])
        for k, v in out.items():
            total[k] = max(total[k], v) if k == "rounds" else total[k] + v
    t0 = time.perf_counter()
    out = sess.punctuate(int(arr["stamp_ms"].max()) + 120000)   # (the traces do not all start at the same second)
    punct = dict(wall_ms=(time.perf_counter() - t0) * 1e3, parts=sess.ms(), counts=out)
    wall_s = (sum(q[0] for q in pushes) + punct["wall_ms"]) * 1e-3   # the calls alone, back to back
    loop_s = time.perf_counter() - t_all
    left = int(sess.store()["cnt"].sum())
    sess.close()
    p = np.array([q[:6] for q in pushes])
    steady = p[len(p) // 6:]   # the first pushes only fill the lists (nothing triggers before 60 s)
    return dict(wall_s=wall_s, points_per_s=len(arr["vehicle"]) / wall_s, counts=total, punctuate=punct, left_in_store=left,
                window_points=matched, loop_s=loop_s,
                sum_ms=dict(zip(("wall",) + PARTS, p.sum(axis=0).round(2).tolist())),
                steady_push_median_ms=dict(zip(("wall",) + PARTS, np.median(steady, axis=0).round(3).tolist())),
                push_columns=["wall_ms"] + list(PARTS) + ["triggers", "rounds", "forwarded"], pushes=pushes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vehicles", type=int, default=10000)
    ap.add_argument("--points", type=int, default=600)
    ap.add_argument("--slice", type=float, default=10.0)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "sessions", "session_probe.json"))
    a = ap.parse_args()
    cfg = world.CONFIGS["C2"]
    tmp = tempfile.mkdtemp(prefix="session_probe")
    graph = os.path.join(tmp, "c2.rmg")
    world.build_world(graph, cfg["rows"], cfg["cols"], cfg["block_m"], seed=1, cell_m=cfg["cell_m"])
    tr = world.generate_traces(graph, n_traces=a.vehicles, n_points=a.points, rate_s=cfg["rate_s"], noise_m=cfg["noise_m"],
                               seed=1000)
    T, n = a.vehicles, a.points
    order = np.arange(T * n).reshape(T, n).T.ravel()          # time-major: every vehicle's k-th point, then the next
    arr = {"vehicle": (order // n).astype(np.uint32)}
    for f in ("time", "lon", "lat", "accuracy"):
        arr[f] = np.ascontiguousarray(tr[f][order])
    arr["stamp_ms"] = (arr["time"] * 1000.0).astype(np.int64)
    per = max(1, int(round(a.slice / cfg["rate_s"]))) * T
    cuts = [(s, min(s + per, T * n)) for s in range(0, T * n, per)]
    veh = np.repeat(np.arange(T, dtype=np.uint32), n)
    eng = engine.Engine(graph, 0)
    bm = engine.BatchMatcher(eng)
    # warm both paths (route tables, workspaces)
    bm.run_points(veh, tr["time"], tr["lon"], tr["lat"], tr["accuracy"], inactivity=120, n_uuids=T)
    stream(bm, arr, cuts[:8], T)
    runs = []
    for _ in range(max(a.runs, 1)):
        s = stream(bm, arr, cuts, T)
        t0 = time.perf_counter()
        bm.run_points(veh, tr["time"], tr["lon"], tr["lat"], tr["accuracy"], inactivity=120, n_uuids=T)
        one = time.perf_counter() - t0
        sz = bm.sizes()
        runs.append(dict(stream=s, run_points=dict(wall_s=one, points_per_s=T * n / one, traces=sz["traces"], reports=sz["reports"])))
    out = dict(vehicles=T, points_per_vehicle=n, slice_s=a.slice, pushes=len(cuts), arrivals_per_push=per, runs=runs,
               stream_points_per_s=[r["stream"]["points_per_s"] for r in runs],
               run_points_points_per_s=[r["run_points"]["points_per_s"] for r in runs],
               replaced_path_points_per_s=11.4e6,
               replaced_path="BENCH_r06.json: 60-point requests through rm_match_batch at 64 clients (not re-measured)")
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    bm.close()
    eng.close()


if __name__ == "__main__":
    main()
