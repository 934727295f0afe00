"""The /report reply measurements (DESIGN.md §3 rule 19): one JSON file per case under
profiles/report/.  Every case repeats (default 5) and keeps every repeat, so ranges can be quoted.

    python scripts/report_probe.py batch        # C2's requests through ReportMany, device and host writer, and MatchMany
    python scripts/report_probe.py interpreted  # what a caller did before: MatchMany, json.loads, report(), json.dumps
    python scripts/report_probe.py service --call report | interpreted   # 64 threads of 60-point requests

`interpreted` and `service --call interpreted` use nothing the Report calls added, so they also run
on a checkout without them (the route they are compared against)."""
import argparse
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import report_oracle  # noqa: E402
import valhalla  # noqa: E402
from reporter_amd import world  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["batch", "interpreted", "service"])
ap.add_argument("--config", default="C2")
ap.add_argument("--traces", type=int, default=0, help="requests (default: the config's)")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--threshold", type=float, default=15.0)
ap.add_argument("--call", default="report", choices=["report", "interpreted"])
ap.add_argument("--clients", type=int, default=64)
ap.add_argument("--requests", type=int, default=8192)
ap.add_argument("--out", default="")
ap.add_argument("--work", default="/tmp/rmprobe")
a = ap.parse_args()

LEVELS = ([0, 1], [0, 1])
c = dict(world.CONFIGS[a.config])
n_traces = a.traces or c["n_traces"]
n_points = 60 if a.mode == "service" else c["n_points"]
os.makedirs(a.work, exist_ok=True)
gp = os.path.join(a.work, "%s.rmg" % a.config)
world.build_config_graph(a.config, gp, seed=1)
tr = world.generate_traces(gp, n_traces if a.mode != "service" else 1024, n_points, c["rate_s"], c["noise_m"], seed=7)
reqs = [json.dumps(world.trace_to_request(tr, k, report_levels=LEVELS[0], transition_levels=LEVELS[1]),
                   separators=(",", ":")).encode() for k in range(len(tr["trace_off"]) - 1)]
points = int(tr["trace_off"][-1])
valhalla.Configure(valhalla.write_config(os.path.join(a.work, "report_probe.json"), gp, device=0, coalesce=True,
                                         search_radius=c["search_radius"]))
out = {"mode": a.mode, "config": a.config, "requests": len(reqs), "points": points, "threshold_sec": a.threshold,
       "request_bytes": sum(len(r) for r in reqs), "repeats": []}


def interpreted(reply, req):
    """py/reporter_service.py:240-243 after Match: json.loads, report(), json.dumps."""
    return json.dumps(report_oracle.report(json.loads(reply), json.loads(req), a.threshold, set(LEVELS[0]), set(LEVELS[1])),
                      separators=(",", ":"))


if a.mode == "batch":
    sm = valhalla.SegmentMatcher()
    sm.ReportMany(reqs, a.threshold)   # untimed: pools and route tables sized
    for rep in range(a.reps):
        row = {}
        for name, limit in (("device", "0"), ("host", "1e18")):
            os.environ["RM_REPLY_DEVICE_MIN_POINTS"] = limit
            t = time.perf_counter()
            replies = sm.ReportMany(reqs, a.threshold)
            wall = time.perf_counter() - t
            row[name] = dict(sm.last_timing(), wall_ms=wall * 1e3, reply_bytes=sum(len(x) for x in replies), **sm.last_report_info())
        t = time.perf_counter()
        sm.MatchMany(reqs)
        row["match_many"] = dict(sm.last_timing(), wall_ms=(time.perf_counter() - t) * 1e3)
        out["repeats"].append(row)
        print(json.dumps(row), flush=True)
elif a.mode == "interpreted":
    sm = valhalla.SegmentMatcher()
    sm.MatchMany(reqs)
    for rep in range(a.reps):
        t = time.perf_counter()
        matched = sm.MatchMany(reqs)
        t1 = time.perf_counter()
        replies = [interpreted(m, r) for m, r in zip(matched, reqs)]
        t2 = time.perf_counter()
        row = dict(sm.last_timing(), match_many_wall_ms=(t1 - t) * 1e3, interpreted_ms=(t2 - t1) * 1e3, wall_ms=(t2 - t) * 1e3,
                   reply_bytes=sum(len(x) for x in replies))
        out["repeats"].append(row)
        print(json.dumps(row), flush=True)
else:
    out["clients"], out["call"] = a.clients, a.call

    def run(lo, hi, lat):
        def client(k):
            m = valhalla.SegmentMatcher()
            for q in range(lo + k, hi, a.clients):
                r = reqs[q % len(reqs)]
                t = time.perf_counter()
                if a.call == "report":
                    m.Report(r, a.threshold)
                else:
                    interpreted(m.Match(r), r)
                lat[k].append(time.perf_counter() - t)
            m.close()
        ths = [threading.Thread(target=client, args=(k,)) for k in range(a.clients)]
        t = time.perf_counter()
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        return time.perf_counter() - t

    run(0, 1024, [[] for _ in range(a.clients)])
    for rep in range(a.reps):
        lat = [[] for _ in range(a.clients)]
        dt = run(1024, 1024 + a.requests, lat)
        all_lat = sorted(x for l in lat for x in l)
        row = {"seconds": dt, "requests": len(all_lat), "points_per_s": len(all_lat) * n_points / dt,
               "p50_ms": all_lat[len(all_lat) // 2] * 1e3, "p99_ms": all_lat[int(len(all_lat) * 0.99)] * 1e3}
        out["repeats"].append(row)
        print(json.dumps(row), flush=True)
    out["coalesce"] = valhalla.coalesce_stats()

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
