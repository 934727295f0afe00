"""Every link of both search-tier chains carrying items in one run, against the oracle (GPU).

The routes stage (K2) and the path stage hand a search that outgrows one tier to the next: ball ->
lane -> reg2 -> 16-lane group -> 512-slot wave -> 4096-slot wave -> global memory.  Two links of a
stage share a list with two others, and the path stage borrows a list of the routes stage, so a
mis-wired list shows only in a run in which every link hands something over.  The other tier tests
see `ball_to_search`, `paths_ball_to_search` and `wave_to_global` above zero in separate runs.

World and batch: an 80 x 80 grid of 100 m blocks (6,400 nodes: a bound of several kilometres labels
more than the 3,072 nodes the 4096-slot hash takes) and one batch of under 2,000 points that mixes,
through per-trace options,
  * 1 s sampling (lane and reg2 tiers),
  * 30 s sampling with a 100 m search radius (group, 512- and 4096-slot tiers),
  * 200 s sampling with breakage_distance 10 km (global-memory tier).

Counters (the tests print them; measured on the commit before the tier kernels became templates,
and the same after it), 8 + 48 + 8 traces, 1,680 points:
  ordinary, radius 0:   lane_to_tier2 11435, tier2_to_wave 11397 (group grid 32 blocks x 4 items = 128),
                        group_to_wave512 4380, wave512_to_wave4096 404, wave_to_global 28;
                        paths: lane -> reg2 1133 (sizes()' paths_tier2), paths_group_to_wave512 640,
                        paths_wave512_to_wave4096 31, paths_wave_to_global 2; both ball counters 0
  ordinary, 60 m balls: ball_to_search 11622, lane_to_tier2 11420, paths_ball_to_search 1131,
                        paths_tier2 1130, the rest as above
  small, short chain:   ball_to_search 11622, group_to_wave512 4380, paths_group_to_wave512 640,
                        wave_to_global 28, paths_wave_to_global 2; lane, reg2 and 512-slot links 0
  small, full chain:    as ordinary with 60 m balls
Without route balls (radius 0) no ball tier runs, so nothing can count its two links in that run:
"every counter above zero" is asserted for the eight others there, and for all ten in the run with
60 m balls (same batch, same oracle answer: the oracle does not depend on the radius).
"""
import numpy as np
import pytest

import meili_oracle as mo
from parity_util import compare_all
from reporter_amd import engine, graphfile, world

pytestmark = pytest.mark.gpu

N_1S, N_30S, N_200S = 8, 48, 8           # traces of each kind ...
P_1S, P_30S, P_200S = 60, 24, 6          # ... and their points: 480 + 1,152 + 48 = 1,680
BALL_RADIUS_M = 60.0
TIER_KEYS = ("ball_to_search", "lane_to_tier2", "tier2_to_wave", "paths_ball_to_search", "wave_to_global",
             "paths_wave_to_global", "group_to_wave512", "paths_group_to_wave512", "wave512_to_wave4096",
             "paths_wave512_to_wave4096")
BALL_KEYS = ("ball_to_search", "paths_ball_to_search")

_cache = {}


def mixture(path, n1=N_1S, n30=N_30S, n200=N_200S):
    """The three kinds of trace in one batch: (traces, options, option set of each trace)."""
    parts = [world.generate_traces(path, n_traces=n, n_points=p, rate_s=r, noise_m=5.0, seed=s)
             for n, p, r, s in ((n1, P_1S, 1.0, 521), (n30, P_30S, 30.0, 522), (n200, P_200S, 200.0, 523))]
    tr = {k: np.concatenate([q[k] for q in parts]) for k in ("lon", "lat", "time", "accuracy")}
    lens = np.concatenate([np.diff(q["trace_off"].astype(np.int64)) for q in parts])
    tr["trace_off"] = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    opts = engine.default_options(3)
    opts[1]["search_radius"] = 100.0
    opts[2]["breakage_distance"] = 10000.0
    trace_opt = np.repeat(np.arange(3, dtype=np.uint32), (n1, n30, n200))
    return tr, opts, trace_opt


def _world(tmpdir_session):
    if "path" not in _cache:
        path = str(tmpdir_session / "tier_chain.rmg")
        world.build_world(path, 80, 80, 100.0, seed=21, cell_m=100.0)
        _cache["path"] = path
    return _cache["path"]


def _case(tmpdir_session):
    """World, batch and the oracle's answer: computed once, shared by the tests, left unchanged."""
    path = _world(tmpdir_session)
    if "ref" not in _cache:
        tr, opts, trace_opt = mixture(path)
        assert int(tr["trace_off"][-1]) <= 2000
        _cache["batch"] = (tr, opts, trace_opt)
        _cache["ref"] = mo.match(graphfile.load(path), mo.Batch(tr["trace_off"], tr["lon"], tr["lat"], tr["time"],
                                                                tr["accuracy"], opts, trace_opt))
    return (path,) + _cache["batch"] + (_cache["ref"],)


def _run(bm, tr, opts, trace_opt):
    bm.run(tr["trace_off"], tr["lon"], tr["lat"], tr["time"], tr["accuracy"], opts, trace_opt)


@pytest.mark.parametrize("radius", [0.0, BALL_RADIUS_M], ids=["radius0", "balls60"])
def test_ordinary_run_every_link_hands_over(built_lib, tmpdir_session, monkeypatch, radius):
    """The ordinary path (the small one forced off): every stage equals the oracle while every link
    of both chains carries items, the group tier's grid-stride loop runs more than once, and a
    rerun on the same matcher (the global tier then runs in line) equals the oracle again."""
    monkeypatch.setenv("RM_SMALL_BATCH_POINTS", "0")
    path, tr, opts, trace_opt, ref = _case(tmpdir_session)
    eng = engine.Engine(path, 0)
    eng.set_ball_radius(radius)
    bm = engine.BatchMatcher(eng)
    _run(bm, tr, opts, trace_opt)
    tiers, sizes = bm.route_tiers(), bm.sizes()
    print("ordinary radius %g" % radius, tiers, "paths_tier2", sizes["paths_tier2"])
    c = compare_all(bm, ref, tr["trace_off"])
    assert c["chained"] > 500, c
    # (without route balls no ball tier runs: nothing can count its two words)
    must = [k for k in TIER_KEYS if radius or k not in BALL_KEYS]
    assert all(tiers[k] > 0 for k in must), tiers
    assert sizes["paths_tier2"] > 0, sizes
    if not radius:
        # the group tier's grid is max(32, P / 64) blocks of four items: more than four grids' worth
        # of items take its grid-stride loop round again
        grid = max(32, int(tr["trace_off"][-1]) // 64)
        assert tiers["tier2_to_wave"] > 4 * 4 * grid, (tiers, grid)
    bm.rerun()
    compare_all(bm, ref, tr["trace_off"])
    assert bm.route_tiers()["wave_to_global"] == tiers["wave_to_global"]
    bm.close()
    eng.close()


def test_small_run_both_chains(built_lib, tmpdir_session, monkeypatch):
    """The small path with 60 m route balls: the short chain (ball -> group -> 4096-slot wave) and
    the full chain (RM_SMALL_SHORT_CHAIN=0) equal the oracle.  (The first run meets the global tier
    before its scratch exists and falls back to the ordinary path, which allocates it.)"""
    monkeypatch.delenv("RM_SMALL_BATCH_POINTS", raising=False)
    path, tr, opts, trace_opt, ref = _case(tmpdir_session)
    eng = engine.Engine(path, 0)
    eng.set_ball_radius(BALL_RADIUS_M)
    bm = engine.BatchMatcher(eng)
    tiers = {}
    for short in (None, None, "0"):
        if short is None:
            monkeypatch.delenv("RM_SMALL_SHORT_CHAIN", raising=False)
        else:
            monkeypatch.setenv("RM_SMALL_SHORT_CHAIN", short)
        _run(bm, tr, opts, trace_opt)
        tiers[short] = bm.route_tiers()
        compare_all(bm, ref, tr["trace_off"])
    print("small short", tiers[None], "full", tiers["0"])
    assert tiers[None]["ball_to_search"] > 0 and tiers[None]["group_to_wave512"] > 0, tiers
    assert tiers[None]["lane_to_tier2"] == 0, tiers   # the short chain: the lane tier did not run
    assert all(tiers["0"][k] > 0 for k in TIER_KEYS), tiers
    bm.close()
    eng.close()
