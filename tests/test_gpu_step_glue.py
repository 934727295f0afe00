"""The steady step's glue (Matcher::run_steady), GPU: scans without a one-block kernel, fill passes
folded into the apply passes, and hand-over tiers left out after clean runs.

A steady run's two scans (transitions / K2 sources, traversal records) take their block bases from
coarse buckets of 64 blocks plus the partials inside the group (rm_common.hpp scan_base_lane; engine.hip
BaseBuckets), the apply passes (k_trans_apply, k_path_apply) also write src_item and rec_slot under local bounds, and a stage's five hand-over
tiers are not launched once two runs in a row handed nothing over -- a prediction checked on the
device every run.  Every run must equal the oracle bit for bit.  RM_SMALL_BATCH_POINTS=0 keeps the
batches off the small-batch path.
"""
import ctypes

import numpy as np
import pytest

import meili_oracle as mo
from parity_util import compare_all
from reporter_amd import _lib, engine, graphfile, world

pytestmark = pytest.mark.gpu

_cache = {}


def _batch(path, n_traces, seed, rate=1.0, n_points=60):
    key = ("tr", n_traces, seed, rate, n_points)
    if key not in _cache:
        _cache[key] = world.generate_traces(path, n_traces=n_traces, n_points=n_points, rate_s=rate, noise_m=5.0,
                                            seed=seed)
    return _cache[key]


def _ref(path, tr_key, tr, opts, turn):
    """The oracle's answer, computed once per (batch, turn factor) and shared by the tests."""
    key = ("ref", tr_key, turn)
    if key not in _cache:
        T = len(tr["trace_off"]) - 1
        _cache[key] = mo.match(graphfile.load(path), mo.Batch(tr["trace_off"], tr["lon"], tr["lat"], tr["time"],
                                                              tr["accuracy"], opts, np.zeros(T, np.uint32)))
    return _cache[key]


def _run(bm, tr, opts, **rp):
    bm.run(tr["trace_off"], tr["lon"], tr["lat"], tr["time"], tr["accuracy"], opts, **rp)
    off, segs = bm.segments()
    return off.tobytes(), segs.tobytes()


# 600 traces x 60 points = 36,000 slots = 141 blocks of 256: two full groups of 64 blocks, a
# partial third group and a partial last block (the record scan: 36 blocks of 1,024, one group)
@pytest.mark.parametrize("turn,locality,radius", [(0.0, 0, None), (200.0, 0, None), (0.0, 2, None), (200.0, 0, 0.0)],
                         ids=["0.0-0", "200.0-0", "0.0-2", "200.0-0-radius0"])
def test_scan_across_groups(built_lib, small_world, monkeypatch, turn, locality, radius):
    """One ordinary run and two steady runs on one matcher: every stage equals the oracle and the
    three runs' segments are the same bytes.  (With the locality order forced the runs stay on the
    ordinary path, whose scans must agree as well.  With ball radius 0 K2 runs entirely in the search
    tiers, with turn costs; the oracle does not depend on the radius.)"""
    monkeypatch.setenv("RM_SMALL_BATCH_POINTS", "0")
    tr = _batch(small_world, 600, 411)
    assert int(tr["trace_off"][-1]) == 36_000
    opts = engine.default_options(1, turn_penalty_factor=turn)
    ref = _ref(small_world, 411, tr, opts, turn)
    eng = engine.Engine(small_world, 0)
    if radius is not None:
        eng.set_ball_radius(radius)
    bm = engine.BatchMatcher(eng)
    if locality:
        bm.set_locality(locality)
    outs = []
    for _ in range(3):
        outs.append(_run(bm, tr, opts))
        c = compare_all(bm, ref, tr["trace_off"])
        assert c["segments"] > 600, c
    assert outs[0] == outs[1] == outs[2]
    st = bm.run_stats()
    print(st)
    assert st["steady"] == (0 if locality else 2) and st["steady_rerun"] == 0, st
    bm.close()
    eng.close()


def test_outgrown_pools(built_lib, small_world, monkeypatch):
    """150 x 60 points, then 600 x 60 on one matcher: the second batch has four times the K2
    sources and records the pools hold, so the fused fills stop at their local bounds, the run is
    gated off and the batch runs again the ordinary way; the large batch then runs steady."""
    monkeypatch.setenv("RM_SMALL_BATCH_POINTS", "0")
    opts = engine.default_options(1)
    small, large = _batch(small_world, 150, 412), _batch(small_world, 600, 411)
    ref_s, ref_l = _ref(small_world, 412, small, opts, 0.0), _ref(small_world, 411, large, opts, 0.0)
    eng = engine.Engine(small_world, 0)
    bm = engine.BatchMatcher(eng)
    want = [(0, 0), (1, 1), (2, 1)]
    outs = []
    for (tr, ref), (steady, rerun) in zip(((small, ref_s), (large, ref_l), (large, ref_l)), want):
        outs.append(_run(bm, tr, opts))
        compare_all(bm, ref, tr["trace_off"])
        st = bm.run_stats()
        print(st)
        assert (st["steady"], st["steady_rerun"]) == (steady, rerun), st
    assert outs[1] == outs[2]
    bm.close()
    eng.close()


def _tier_sequence(path, clean, ref_c, sparse, ref_s, opts):
    eng = engine.Engine(path, 0)
    eng.set_ball_radius(300.0)   # well below the sparse batch's route bounds, above the clean batch's
    bm = engine.BatchMatcher(eng)
    bm.set_locality(0)   # (a sparsely sampled batch would otherwise take the locality order, not a steady run)
    outs, stats = [], []

    def step(tr, ref):
        outs.append(_run(bm, tr, opts))
        compare_all(bm, ref, tr["trace_off"])
        stats.append(bm.run_stats())
        return bm.route_tiers()

    for _ in range(4):   # ordinary, steady with the tiers, then two runs without them
        t = step(clean, ref_c)
        assert not any(t.values()), t
    t = step(sparse, ref_s)   # hands over: detected on the device, run again the ordinary way
    assert t["ball_to_search"] > 0, t
    paths_handed = t["paths_ball_to_search"] > 0
    step(sparse, ref_s)       # steady, the tiers launched
    for _ in range(3):        # two clean runs re-arm the skipping, the third skips again
        step(clean, ref_c)
    bm.close()
    eng.close()
    return outs, stats, paths_handed


def test_tier_skipping(built_lib, small_world, monkeypatch):
    """A batch without hand-overs four times, one that hands over twice, the clean one three times
    more: every run equals the oracle, the tiers are left out from the third clean run on, the
    batch that hands over is detected and run again, and RM_STEADY_TIERS=0 (tiers always launched)
    gives the same bytes."""
    monkeypatch.setenv("RM_SMALL_BATCH_POINTS", "0")
    opts = engine.default_options(1)
    clean = _batch(small_world, 150, 412)
    sparse = _batch(small_world, 150, 413, rate=30.0)
    ref_c, ref_s = _ref(small_world, 412, clean, opts, 0.0), _ref(small_world, 413, sparse, opts, 0.0)
    monkeypatch.setenv("RM_STEADY_TIERS", "1")
    outs, stats, paths_handed = _tier_sequence(small_world, clean, ref_c, sparse, ref_s, opts)
    print(stats, paths_handed)
    skipped = [(s["routes_tiers_skipped"], s["paths_tiers_skipped"]) for s in stats]
    assert skipped[:4] == [(0, 0), (0, 0), (1, 1), (2, 2)], skipped
    # the sparse batch: one more steady run without the routes tiers, gated off and run again
    assert stats[4]["steady_rerun"] == stats[3]["steady_rerun"] + 1, stats
    assert stats[4]["routes_tiers_skipped"] == 3, stats
    # its second run and the next two clean runs launch the routes tiers; the third clean run does not
    assert [s["routes_tiers_skipped"] for s in stats[5:]] == [3, 3, 3, 4], stats
    if paths_handed:
        assert [s["paths_tiers_skipped"] for s in stats[4:]] == [3, 3, 3, 3, 4], stats
    monkeypatch.setenv("RM_STEADY_TIERS", "0")
    outs0, stats0, _ = _tier_sequence(small_world, clean, ref_c, sparse, ref_s, opts)
    assert stats0[-1]["routes_tiers_skipped"] == 0 and stats0[-1]["paths_tiers_skipped"] == 0, stats0
    assert outs == outs0


def test_steady_histogram_is_zeroed(built_lib, small_world, monkeypatch):
    """Two steady runs with the speed histogram and zero_hist: the second run's histogram and
    duration sums equal the oracle's for one batch (a missed or late zeroing would add to them)."""
    monkeypatch.setenv("RM_SMALL_BATCH_POINTS", "0")
    opts = engine.default_options(1)
    tr = _batch(small_world, 150, 412)
    T = len(tr["trace_off"]) - 1
    g = graphfile.load(small_world)
    eng = engine.Engine(small_world, 0)
    nseg = eng.n_segments
    want = np.zeros(nseg * 16, np.uint32)
    want_dur = np.zeros(nseg, np.uint64)
    batch = mo.Batch(tr["trace_off"], tr["lon"], tr["lat"], tr["time"], tr["accuracy"], opts, np.zeros(T, np.uint32))
    nvalid = mo.pipeline(g, batch, 15.0, engine.levels_mask((0, 1)), engine.levels_mask((0, 1)), want, want_dur)
    assert nvalid > 0
    L = _lib.lib()
    dptr, uptr = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.check(L.rm_device_alloc(nseg * 16 * 4, ctypes.byref(dptr)))
    _lib.check(L.rm_device_alloc(nseg * 8, ctypes.byref(uptr)))
    try:
        bm = engine.BatchMatcher(eng)
        for run in range(3):   # ordinary, steady, steady
            _run(bm, tr, opts, hist_dev=dptr.value, dur_dev=uptr.value, zero_hist=True)
            got = np.empty(nseg * 16, np.uint32)
            got_dur = np.empty(nseg, np.uint64)
            _lib.check(L.rm_device_download(got.ctypes.data, dptr, got.nbytes))
            _lib.check(L.rm_device_download(got_dur.ctypes.data, uptr, got_dur.nbytes))
            np.testing.assert_array_equal(got, want, "speed histogram, run %d" % run)
            np.testing.assert_array_equal(got_dur, want_dur, "duration sums, run %d" % run)
        assert bm.run_stats()["steady"] == 2
        bm.close()
    finally:
        L.rm_device_free(dptr)
        L.rm_device_free(uptr)
        eng.close()
