"""Matched points (DESIGN.md §3 rule 9): the independent restatement against the oracle and the
generator's truth (CPU), and the C-ABI additions.

The reference (tests/matched_points_ref.py) places every input point of the C1-sized trace sets on
the road from the oracle's outputs.  Its frame is pinned by the oracle (a state point projected
onto its chosen road reproduces cand_sq bit for bit), its records are checked for the rule's
structural properties, and its accuracy is measured in metres against the road position the
trace generator drove (truth_edge / truth_off_cm) -- which GPU/oracle bit-parity cannot show.

Share of points within 10 m of the truth at 5 m of noise (bounds from the issue: a float64
prototype of the rule gave 99.71 / 99.80 % at 1 Hz and 99.17 / 99.06 % at 4 Hz):

    set     type 1 (states)   type 2 (interpolated)   bound    medians
    1 Hz    99.71 %           99.70 %                 >= 99 %  4.07 m / 4.06 m
    4 Hz    99.17 %           99.06 %                 >= 98 %  3.85 m / 3.91 m

Non-state points: 42.2 % of the 1 Hz set (bound >= 35 %), 80.0 % of the 4 Hz set (>= 70 %).
"""
import ctypes

import numpy as np
import pytest

import matched_points_ref as mp
import meili_oracle as mo
from reporter_amd import engine, graphfile, world

SETS = {"1hz": dict(n_points=60, rate_s=1.0, within=0.99, share=0.35),
        "4hz": dict(n_points=120, rate_s=0.25, within=0.98, share=0.70)}


@pytest.fixture(scope="module", params=sorted(SETS))
def placed(request, small_world):
    """(set parameters, graph, Roads, traces, oracle outputs, reference records), computed once."""
    cfg = SETS[request.param]
    g = graphfile.load(small_world)
    tr = world.generate_traces(small_world, n_traces=40, n_points=cfg["n_points"], rate_s=cfg["rate_s"], noise_m=5.0,
                               seed=301)
    opts = engine.default_options(1)
    topt = np.zeros(40, np.uint32)
    ref = mo.match(g, mo.Batch(tr["trace_off"], tr["lon"], tr["lat"], tr["time"], tr["accuracy"], opts, topt))
    R = mp.Roads(g)
    rec = mp.matched_points(g, tr, opts, topt, ref, R=R)
    return cfg, g, R, tr, ref, rec


def _state_points(tr, ref):
    """Per point: its state slot (or -1), and the slot of the state at or before it."""
    P = int(tr["trace_off"][-1])
    slot = np.full(P, -1, np.int64)
    owner = np.full(P, -1, np.int64)
    for k in range(len(tr["trace_off"]) - 1):
        o, n = int(tr["trace_off"][k]), int(tr["trace_off"][k + 1] - tr["trace_off"][k])
        S = int(ref["n_states"][k])
        so = ref["state_orig"][o:o + S].astype(np.int64)
        slot[o + so] = o + np.arange(S)
        owner[o:o + n] = o + np.searchsorted(so, np.arange(n), side="right") - 1
    return slot, owner


def test_frame_is_pinned_by_the_oracle(placed):
    """K1's projection restated: sq bits == cand_sq and s == cand_s for every chosen candidate."""
    cfg, g, R, tr, ref, rec = placed
    assert mp.check_frame(g, tr, ref, R) == int((rec["type"] == mp.MATCHED).sum()) > 900


def test_record_structure(placed):
    cfg, g, R, tr, ref, rec = placed
    P = int(tr["trace_off"][-1])
    assert len(rec) == P and rec.dtype.itemsize == 32                  # one record per point
    slot, owner = _state_points(tr, ref)
    is_state = slot >= 0
    chosen = np.zeros(P, bool)
    chosen[is_state] = ref["choice"][slot[is_state]] >= 0
    np.testing.assert_array_equal(rec["type"] == mp.MATCHED, chosen)   # type 1 exactly on the chosen states
    follows = ~is_state & (ref["choice"][owner] >= 0)
    np.testing.assert_array_equal(rec["type"] == mp.INTERPOLATED, follows)
    un = rec["type"] == mp.UNMATCHED
    assert (rec["edge"][un] == mp.NONE).all()
    for f in ("lon", "lat", "sq", "off_cm", "way", "route_cm"):
        assert not rec[f][un].any(), f
    assert not rec["route_cm"][rec["type"] == mp.MATCHED].any()
    share = 1.0 - is_state.sum() / P
    print("non-state share %.4f" % share)
    assert share >= cfg["share"]
    # every record lies on its edge and carries its way
    m = ~un
    e = rec["edge"][m].astype(np.int64)
    elen = g["edges"].reshape(-1, 4)[e, 1]
    assert (rec["off_cm"][m] <= elen).all()
    np.testing.assert_array_equal(rec["way"][m], g["edge_way"][e])


def test_gap_points_follow_the_clipped_path(placed):
    """route_cm never decreases inside a gap and never exceeds the transition's route_dist; every
    type-2 (edge, off_cm) lies on a piece of the transition's path, clipped at both candidates."""
    cfg, g, R, tr, ref, rec = placed
    slot, owner = _state_points(tr, ref)
    seen = 0
    for p in np.nonzero(rec["type"] == mp.INTERPOLATED)[0]:
        a = int(owner[p])
        prev = 0 if slot[p - 1] >= 0 else int(rec["route_cm"][p - 1])
        x = int(rec["route_cm"][p])
        assert x >= prev, (p, x, prev)
        e, c = int(rec["edge"][p]), int(rec["off_cm"][p])
        k = int(np.searchsorted(tr["trace_off"], p, side="right") - 1)
        o, S = int(tr["trace_off"][k]), int(ref["n_states"][k])
        l = a + 1
        chained = l - o < S and not ref["chain_start"][l] and ref["choice"][l] >= 0
        if chained:
            assert x <= int(ref["route_dist"][l]), (p, x)
            po, pn = int(ref["path_off"][l]), int(ref["path_cnt"][l])
            sa = int(ref["cand_s"][a, ref["choice"][a]])
            sb = int(ref["cand_s"][l, ref["choice"][l]])
            x0, ok = 0, False
            for q in range(pn):
                pe = int(ref["path_pool"][po + q])
                L, rv = R.len[R.e_road[pe]], R.e_rev[pe]
                c0 = (L - sa if rv else sa) if q == 0 else 0
                c1 = (L - sb if rv else sb) if q + 1 == pn else L
                ok |= pe == e and c0 <= c <= c1 and x == x0 + c - c0
                x0 += c1 - c0
            assert ok, (p, e, c, x)
            seen += 1
        else:   # the chain ends at the state: the rest of its own edge
            sp = o + int(ref["state_orig"][a])   # the state's own point
            assert e == int(rec["edge"][sp]), p
            so = int(rec["off_cm"][sp])
            assert c >= so and x == c - so and c <= R.len[R.e_road[e]], (p, c, so, x)
    assert seen > 500


def test_accuracy_against_the_generator(placed):
    cfg, g, R, tr, ref, rec = placed
    d = mp.truth_distance_m(g, tr, rec, R)
    for t in (mp.MATCHED, mp.INTERPOLATED):
        m = rec["type"] == t
        within = float((d[m] <= 10.0).mean())
        print("type %d: %d points, %.2f %% within 10 m, median %.2f m" % (t, m.sum(), 100 * within, np.median(d[m])))
        assert m.sum() > 900
        assert within >= cfg["within"], (t, within)
        assert np.median(d[m]) < 5.0
    # the snapped position is where sq says it is: sqrt(sq) against the fp64 distance to the measurement
    m = rec["type"] != mp.UNMATCHED
    dx = (rec["lon"][m].astype(np.float64) - tr["lon"][m].astype(np.float32)) * 111320.0 * np.cos(
        np.radians(tr["lat"][m].astype(np.float32).astype(np.float64)))
    dy = (rec["lat"][m].astype(np.float64) - tr["lat"][m].astype(np.float32)) * 110567.0
    np.testing.assert_allclose(np.sqrt(rec["sq"][m].astype(np.float64)), np.hypot(dx, dy), rtol=1e-4, atol=1e-3)


def test_abi_additions(built_lib):
    """The 32-byte record and the three new calls exist in the built library and its binding."""
    from reporter_amd import _lib
    assert ctypes.sizeof(_lib.RmMatchedPoint) == 32 == engine.MATCHED_POINT_DTYPE.itemsize == mp.REC.itemsize
    assert [n for n, _ in _lib.RmMatchedPoint._fields_] == list(engine.MATCHED_POINT_DTYPE.names) == list(mp.REC.names)
    h = ctypes.CDLL(built_lib)
    for name in ("rm_runner_get_matched_points", "rm_match_points", "rm_match_points_batch"):
        assert hasattr(h, name), name
    assert _lib.lib().rm_abi_version() == 1   # additive: the ABI version stays
    names = [_lib.lib().rm_kernel_name(i).decode() for i in range(_lib.lib().rm_num_kernels())]
    assert names[-1] == "points" and names.index("points") == 9
