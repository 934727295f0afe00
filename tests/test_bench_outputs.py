"""bench.py --dump-outputs / --full: the dump holds what the timed step computed, stays inside
its byte budget by a seeded row sample, and a plain run prints the headline line only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _FakeMatcher:
    """segments() / reports() of engine.BatchMatcher over fixed records."""

    def __init__(self, n_traces, n_seg, n_rep, seed):
        from reporter_amd import engine
        rng = np.random.default_rng(seed)
        self.seg_off = np.linspace(0, n_seg, n_traces + 1).astype(np.uint32)
        self.rep_off = np.linspace(0, n_rep, n_traces + 1).astype(np.uint32)
        self.segs = np.zeros(n_seg, engine.SEGMENT_DTYPE)
        self.segs["segment_id"] = rng.integers(0, 1 << 46, n_seg, dtype=np.uint64)
        self.segs["start_time"] = rng.random(n_seg) * 1e9
        self.segs["length"] = rng.integers(-1, 5000, n_seg)
        self.reps = np.zeros(n_rep, engine.REPORT_DTYPE)
        self.reps["id"] = rng.integers(0, 1 << 46, n_rep, dtype=np.uint64)
        self.reps["t1"] = rng.random(n_rep) * 1e9
        self.stats = np.zeros(n_traces, engine.STATS_DTYPE)
        self.stats["n_reports"] = np.diff(self.rep_off.astype(np.int64))

    def segments(self):
        return self.seg_off, self.segs

    def reports(self):
        return self.rep_off, self.reps, self.stats


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_dump_whole_arrays(built_lib, tmp_path):
    import bench
    from reporter_amd import engine
    bm = _FakeMatcher(7, 100, 40, seed=1)
    hist = np.arange(5 * 16, dtype=np.uint32)
    dur = np.arange(5, dtype=np.uint64) * 3
    bench.dump_outputs(str(tmp_path / "o"), bm, hist, dur)
    got = _load(str(tmp_path / "o"))
    assert sorted(got) == ["duration_sum", "histogram", "report_offsets", "reports", "segment_offsets", "segments",
                           "trace_stats"]
    assert all(v.dtype == np.float64 for v in got.values())
    assert np.array_equal(got["histogram"], hist.reshape(5, 16))
    assert np.array_equal(got["duration_sum"], dur)
    assert np.array_equal(got["segment_offsets"], bm.seg_off)
    assert np.array_equal(got["report_offsets"], bm.rep_off)
    for j, nm in enumerate(engine.SEGMENT_DTYPE.names):
        assert np.array_equal(got["segments"][:, j], bm.segs[nm].astype(np.float64)), nm
    rep_names = [n for n in engine.REPORT_DTYPE.names if n != "pad"]
    assert got["reports"].shape == (40, len(rep_names))
    assert np.array_equal(got["reports"][:, 0].astype(np.uint64), bm.reps["id"])   # 46-bit ids are exact
    assert np.array_equal(got["trace_stats"][:, -1], bm.stats["n_reports"])


def test_dump_samples_within_budget(built_lib, tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 40_000)
    bm = _FakeMatcher(50, 3000, 1000, seed=2)   # segments alone: 3000 x 11 x 8 = 264 kB
    hist = np.arange(300 * 16, dtype=np.uint32)
    dur = np.arange(300, dtype=np.uint64)
    dirs = [str(tmp_path / n) for n in ("a", "b")]
    for d in dirs:
        bench.dump_outputs(d, bm, hist, dur)
    a, b = _load(dirs[0]), _load(dirs[1])
    assert sum(v.nbytes for v in a.values()) <= 40_000
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)   # the same sample every time
    full = {"segments": np.stack([bm.segs[n].astype(np.float64) for n in bm.segs.dtype.names], axis=1),
            "histogram": hist.reshape(-1, 16).astype(np.float64)}
    for name, whole in full.items():
        rows = a[name + "_rows"].astype(np.int64)
        assert 0 < len(rows) < len(whole) and np.all(np.diff(rows) > 0)
        assert np.array_equal(a[name], whole[rows])
    assert "duration_sum_rows" not in a and np.array_equal(a["duration_sum"], dur)   # small arrays stay whole
    # a later dump that fits leaves no stale row indices behind
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 60_000_000)
    bench.dump_outputs(dirs[0], bm, hist, dur)
    assert not [k for k in _load(dirs[0]) if k.endswith("_rows")]


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "C1", "--traces", "8",
                        "--steps", "3", "--warmup", "1"] + list(args), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_what_the_step_computes(built_lib, tmp_path):
    """One plain run in its own process; this process then builds the same seeded inputs and runs
    the engine on them: the dump must hold exactly these outputs (so the inputs are the same
    from run to run, and the files are what a caller of the step receives)."""
    import bench
    from reporter_amd import dist, engine, world as W
    d = str(tmp_path / "dump")
    o = _bench("--dump-outputs", d)
    assert o["steps"] == 3 and o["warmup"] == 1 and o["ms_per_step"] > 0 and o["unit"] == "points/s"
    assert o["higher_is_better"] is True and o["full"] is False
    assert abs(o["value"] - o["config"]["points_all_ranks"] / (o["ms_per_step"] * 1e-3)) <= 1e-6 * o["value"]
    # nothing beyond the headline figure was measured
    assert not {"cpu_baseline", "roofline", "rooflines", "ms_allreduce", "turn_costs", "c1_latency",
                "json_boundary", "concurrent_parts"} & set(o)
    a = _load(d)
    assert sum(v.nbytes for v in a.values()) <= 64 * 1000 * 1000
    assert all(v.dtype == np.float64 for v in a.values())

    cfg = W.CONFIGS["C1"]
    gpath = str(tmp_path / "c1.rmg")
    W.build_config_graph("C1", gpath, seed=1)
    ids = bench.shard_ids("C1", 8, cfg["n_points"], 1, 0)
    tr = W.generate_traces(gpath, 0, cfg["n_points"], cfg["rate_s"], cfg["noise_m"], seed=1000, ids=ids)
    eng = engine.Engine(gpath, 0)
    bm = engine.BatchMatcher(eng)
    nseg = eng.n_segments
    hist, dur = dist.DeviceBuffer(nseg * 16 * 4), dist.DeviceBuffer(nseg * 8)
    try:
        bm.run(tr["trace_off"], tr["lon"], tr["lat"], tr["time"], tr["accuracy"],
               engine.default_options(1, search_radius=cfg["search_radius"]), None,
               hist_dev=hist.ptr, dur_dev=dur.ptr, zero_hist=True)
        seg_off, segs = bm.segments()
        rep_off, reps, stats = bm.reports()
        h, du = hist.download(), dur.download(np.uint64)
    finally:
        hist.close()
        dur.close()
        bm.close()
        eng.close()
    assert len(segs) > 0 and len(reps) > 0 and h.sum() > 0
    assert np.array_equal(a["histogram"], h.reshape(-1, 16))
    assert np.array_equal(a["duration_sum"], du)
    assert np.array_equal(a["segment_offsets"], seg_off) and np.array_equal(a["report_offsets"], rep_off)
    for j, nm in enumerate(engine.SEGMENT_DTYPE.names):
        assert np.array_equal(a["segments"][:, j], segs[nm].astype(np.float64)), nm
    for j, nm in enumerate(n for n in engine.REPORT_DTYPE.names if n != "pad"):
        assert np.array_equal(a["reports"][:, j], reps[nm].astype(np.float64)), nm
    for j, nm in enumerate(engine.STATS_DTYPE.names):
        assert np.array_equal(a["trace_stats"][:, j], stats[nm].astype(np.float64)), nm
    assert a["histogram"].sum() == o["histogram_total"] and a["duration_sum"].sum() == o["duration_sum_total_s"]
    assert len(a["segments"]) == o["sizes_rank0"]["segments"] and len(a["reports"]) == o["sizes_rank0"]["reports"]
