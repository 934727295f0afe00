"""K1's cooperative epilogue: the lane tier stages a wave's candidates in LDS and builds their
descriptors a lane per candidate (engine.hip k_candidates_lane).

Every case runs the C1 world with a batch above 4,096 points, so the lane tier runs (below that
K1 is one wave per state), and compares with the oracle: candidates bit for bit and, through
routes, entry times, paths and segments, every descriptor field.  The asserts on the oracle's
own cand_n make sure the batch really holds what the case is about.
"""
import numpy as np
import pytest

import meili_oracle as mo
from parity_util import check_reports, compare_all, match_and_compare, state_slots
from reporter_amd import engine, graphfile, world

pytestmark = pytest.mark.gpu

K1_STAGE = 384        # engine.hip RM_K1_STAGE: staged records per wave and flush pass
K1_SLOTS = 16         # engine.hip RM_K1_SLOTS: roads a lane keeps; more go to the wave tier
LANE_TIER_MIN = 4096  # engine.hip kSmallWaveK1
RADII = (5.0, 50.0, 120.0, 220.0)   # 220 is clamped to the 200 m maximum


def _mixed_batch(path):
    tr = world.generate_traces(path, n_traces=400, n_points=19, rate_s=1.0, noise_m=5.0, seed=31)
    opts = np.concatenate([engine.default_options(1, search_radius=r) for r in RADII])
    trace_opt = (np.arange(400) % len(RADII)).astype(np.uint32)
    return tr, opts, trace_opt


def _state_n(ref, tr):
    """The oracle's cand_n per point slot, 0 where the slot holds no state."""
    sm = state_slots(tr["trace_off"], ref["n_states"])
    return ref["cand_n"].astype(np.int64) * sm


def _group_totals(n):
    """Candidates of each aligned group of 64 slots: one wave of the lane tier in slot order."""
    pad = (-len(n)) % 64
    return np.concatenate([n, np.zeros(pad, np.int64)]).reshape(-1, 64).sum(1)


def _roads_within(g, lon, lat, radius_m):
    """Distinct roads surely nearer than radius_m to the point: fp64 point-to-piece distances in
    the matcher's local metric frame, independent of the oracle and engine."""
    v = g["verts"].reshape(-1, 4)
    vx = v[:, 0].view(np.float32).astype(np.float64)
    vy = v[:, 1].view(np.float32).astype(np.float64)
    a = np.nonzero(v[:-1, 3] != 0xFFFFFFFF)[0]
    mlon = 111320.0 * np.cos(np.deg2rad(lat))
    ax, ay = (vx[a] - lon) * mlon, (vy[a] - lat) * 110567.0
    bx, by = (vx[a + 1] - lon) * mlon, (vy[a + 1] - lat) * 110567.0
    dx, dy = bx - ax, by - ay
    l2 = dx * dx + dy * dy
    t = np.clip(np.where(l2 > 0, -(ax * dx + ay * dy) / np.where(l2 > 0, l2, 1.0), 0.0), 0.0, 1.0)
    d = np.hypot(ax + t * dx, ay + t * dy)
    return len(np.unique(v[a, 3][d < radius_m]))


def _assert_mixed(g, tr, ref, trace_opt):
    P = len(tr["lon"])
    assert LANE_TIER_MIN < P < 10_000 and P % 64 and P % 256
    n = _state_n(ref, tr)
    sm = state_slots(tr["trace_off"], ref["n_states"])
    assert (n[sm] == 0).any(), "no state without candidates"
    assert (n[sm] == K1_SLOTS).any(), "no state with 16 candidates"
    # a state the lane tier hands to the wave tier: more than 16 roads inside its radius.  The
    # oracle keeps the nearest 16 of them, so its count stops at 16; that more lie inside is
    # shown by counting the roads nearer than the radius less 5 m (far above any rounding)
    slot_opt = np.repeat(trace_opt, np.diff(tr["trace_off"]).astype(np.int64))
    full = np.nonzero(sm & (n == K1_SLOTS) & (slot_opt == 3))[0]
    assert len(full)
    off = np.asarray(tr["trace_off"], np.int64)
    k = np.searchsorted(off, full[0], side="right") - 1
    pt = off[k] + int(ref["state_orig"][full[0]])
    assert _roads_within(g, float(tr["lon"][pt]), float(tr["lat"][pt]), 200.0 - 5.0) > K1_SLOTS
    # one wave holds small and large n side by side
    grp = np.concatenate([n, np.zeros((-P) % 64, np.int64)]).reshape(-1, 64)
    assert ((grp.max(1) >= 12) & ((grp > 0).sum(1) > (grp >= 12).sum(1))).any()


@pytest.fixture(scope="module")
def mixed(small_world):
    tr, opts, trace_opt = _mixed_batch(small_world)
    g = graphfile.load(small_world)
    ref = mo.match(g, mo.Batch(tr["trace_off"], tr["lon"], tr["lat"], tr["time"], tr["accuracy"], opts, trace_opt))
    _assert_mixed(g, tr, ref, trace_opt)
    return tr, opts, trace_opt, ref


def test_mixed_n_inside_one_wave(small_world, mixed):
    """1. 400 traces of 19 points whose search radius cycles 5 / 50 / 120 / 200 m: states with no
    candidate, with 16, and with more roads than the lane tier keeps (wave-tier hand-overs that
    stay in their wave with n = 0) share waves with ordinary ones."""
    tr, opts, trace_opt, _ = mixed
    c = match_and_compare(small_world, tr, opts, trace_opt, keep_ref=True)
    _assert_mixed(graphfile.load(small_world), tr, c.pop("_ref"), trace_opt)
    assert c["chained"] > 1000 and c["segments"] > 100, c
    print("mixed n", c)


def test_several_flush_passes(small_world):
    """2. Radius 150 m: 10 roads or more almost everywhere, so waves hold far more candidates than
    the LDS stage and flush it in several passes, the last one partly filled."""
    tr = world.generate_traces(small_world, n_traces=400, n_points=19, rate_s=1.0, noise_m=5.0, seed=31)
    opts = engine.default_options(1, search_radius=150.0)
    c = match_and_compare(small_world, tr, opts, None, keep_ref=True)
    tot = _group_totals(_state_n(c.pop("_ref"), tr))
    assert tot.max() > K1_STAGE and (tot[tot > K1_STAGE] % K1_STAGE != 0).any(), tot.max()
    assert c["chained"] > 1000, c
    print("flush passes", c, "largest wave total", tot.max())


def test_locality_order_on(small_world, mixed):
    """3. The data of case 1 in locality order: the owner's slot comes from the permutation."""
    tr, opts, trace_opt, ref = mixed
    eng = engine.Engine(small_world, 0)
    bm = engine.BatchMatcher(eng)
    bm.set_locality(1)
    bm.run(tr["trace_off"], tr["lon"], tr["lat"], tr["time"], tr["accuracy"], opts, trace_opt)
    assert bm.locality_used()
    c = compare_all(bm, ref, tr["trace_off"])
    check_reports(bm, ref, tr)
    assert c["chained"] > 1000, c
    bm.close()
    eng.close()


def test_modes_mixed_per_trace(small_world):
    """4. auto / bicycle / pedestrian traces side by side in the waves: the descriptor's speeds
    and entry times depend on the owner's mode, which travels with each staged record."""
    parts, opts = [], []
    for mi, mode in enumerate(("auto", "bicycle", "pedestrian")):
        for si, sz in enumerate((2.0, 4.07, 8.0, 16.0)):
            parts.append(world.generate_traces(small_world, n_traces=20, n_points=19, rate_s=1.0, noise_m=sz,
                                               seed=100 + mi * 10 + si, mode=mode))
            opts.append(engine.default_options(1, mode=world.MODES[mode], sigma_z=sz,
                                               search_radius=max(50.0, 3 * sz))[0])
    tr = {k: np.concatenate([p[k] for p in parts]) for k in ("lon", "lat", "time", "accuracy")}
    T = len(parts) * 20
    k = np.arange(T)
    trace_opt = (k % len(parts)).astype(np.uint32)   # neighbouring traces differ in mode
    src = (k % len(parts)) * 20 + k // len(parts)    # batch trace k: trace k // 12 of part k % 12
    idx = (src[:, None] * 19 + np.arange(19)[None, :]).ravel()
    tr = {f: tr[f][idx] for f in tr}
    tr["trace_off"] = (np.arange(T + 1) * 19).astype(np.uint32)
    assert LANE_TIER_MIN < len(tr["lon"]) < 10_000
    c = match_and_compare(small_world, tr, np.array(opts, engine.OPTIONS_DTYPE), trace_opt,
                          rl=(0, 1, 2), tl=(0, 1, 2))
    assert c["chained"] > 500, c
    print("mixed modes", c)


@pytest.mark.parametrize("path_kind", ["small", "ordinary"])
def test_rerun_gives_identical_candidates(small_world, mixed, monkeypatch, path_kind):
    """5. run, then rerun twice: candidates() identical each time, on the small-batch path and on
    the ordinary plan (RM_SMALL_BATCH_POINTS=0)."""
    if path_kind == "ordinary":
        monkeypatch.setenv("RM_SMALL_BATCH_POINTS", "0")
    else:
        monkeypatch.delenv("RM_SMALL_BATCH_POINTS", raising=False)
    tr, opts, trace_opt, ref = mixed
    eng = engine.Engine(small_world, 0)
    bm = engine.BatchMatcher(eng)
    bm.run(tr["trace_off"], tr["lon"], tr["lat"], tr["time"], tr["accuracy"], opts, trace_opt)
    compare_all(bm, ref, tr["trace_off"])
    first = [np.asarray(a).tobytes() for a in bm.candidates()]
    for _ in range(2):
        bm.rerun()
        assert [np.asarray(a).tobytes() for a in bm.candidates()] == first
    compare_all(bm, ref, tr["trace_off"])
    bm.close()
    eng.close()
