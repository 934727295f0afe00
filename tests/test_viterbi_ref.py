"""The K3 input sets do what they claim (no GPU).

For every set of tests/viterbi_sets.py the oracle runs, tests/viterbi_ref.py (K3 written from the
specification alone) must give the oracle's choice and chain_start on every state slot, and the
reference's coverage record must meet the conditions below: every branch of k_viterbi and
k_viterbi_w that depends on the candidate counts of two adjacent layers, on the chunk layout, on
where a chain ends and on a tie is reached often enough that a set which drifts away from one fails
here.  The conditions are requirements on the inputs: a seed that misses one is changed, not the
threshold."""
from fractions import Fraction

import numpy as np
import pytest

import meili_oracle as mo
import viterbi_ref as vr
import viterbi_sets as vs
from reporter_amd import graphfile


@pytest.fixture(scope="module")
def dense(built_lib, tmp_path_factory):
    path = vs.dense_world(str(tmp_path_factory.mktemp("vit") / "dense.rmg"))
    return dict(path=path, g=graphfile.load(path), cache={})


def covered(dense, name):
    """The set, the oracle's outputs, the reference's and the batch coverage (computed once)."""
    if name not in dense["cache"]:
        s = vs.build(name, dense["path"])
        tr = s["tr"]
        ref = mo.match(dense["g"], mo.Batch(tr["trace_off"], tr["lon"], tr["lat"], tr["time"], tr["accuracy"],
                                            s["opts"], s["topt"]))
        turns = bool((s["opts"]["turn_penalty_factor"] > 0).any())
        assert turns == name.endswith("_turns") and turns == bool(ref["route_turn"].any())
        st = dict(ref, route_d=ref["route_d"] if turns else None)
        choice, cs, covs = vr.run(tr["trace_off"], st, s["opts"], s["topt"])
        tot = vr.total(covs)
        print("K3 coverage", name, "traces", len(tr["trace_off"]) - 1, "points", len(tr["lon"]), vr.summary(tot))
        dense["cache"][name] = dict(set=s, ref=ref, choice=choice, cs=cs, covs=covs, tot=tot)
    return dense["cache"][name]


# ---- the reference itself

def test_fma_rounds_once():
    a, b, c = 1.0 + 2.0 ** -30, 1.0 + 2.0 ** -30, -1.0
    assert a * b + c == 2.0 ** -29                       # two roundings lose the 2^-60 term
    assert vr.fma(a, b, c) == 2.0 ** -29 + 2.0 ** -60    # one keeps it
    assert vr.fma(0.1, 3.0, 0.5) == float(Fraction(0.1) * 3 + Fraction(0.5))


def test_chunk_layout():
    # 16 layers at most; the route limit cuts before the layer that no longer fits
    assert vr.chunk_layout([0] + [4] * 39, 256)[1] == [16] * 32 + [8] * 8
    pos, length, cut = vr.chunk_layout([0, 256, 256, 100, 100, 100], 384)
    assert (pos, length, cut) == ([0, 1, 0, 1, 0, 1], [2, 2, 2, 2, 2, 2], 2)
    pos, length, cut = vr.chunk_layout([0, 256, 256, 100, 100, 100], 256)
    assert (pos, length, cut) == ([0, 1, 0, 0, 1, 0], [2, 2, 1, 2, 2, 1], 3)


def _tiny(routes, sq, gc=(0.0, 10.0), brk=2000.0):
    """Two layers of two candidates."""
    opts = np.zeros(1, [("sigma_z", "<f4"), ("beta", "<f4"), ("breakage_distance", "<f4")])
    opts[0] = (4.0, 3.0, brk)
    sqa = np.zeros((2, 16), np.float32)
    sqa[:, :2] = sq
    return vr.viterbi_ref([0, 2], [2], np.array([2, 2], np.uint8), sqa, np.array([0, 0], np.uint32),
                          np.array(gc), np.array(routes, np.uint32), None, opts)


def test_tie_rules_and_starts():
    # every cost equal: the lowest j wins the chain, its lowest source i the layer before
    choice, cs, covs = _tiny([1000] * 4, [[0, 0], [0, 0]])
    assert choice.tolist() == [0, 0] and cs.tolist() == [1, 0]
    assert covs[0]["source_ties"] == 1 and covs[0]["winner_ties"] == 1
    # the better emission wins; its route from source 1 alone is valid
    bad = vr.ROUTE_INVALID
    choice, cs, covs = _tiny([bad, bad, 1000, 1000], [[0, 0], [5, 1]])
    assert choice.tolist() == [1, 1] and cs.tolist() == [1, 0] and covs[0]["source_ties"] == 0
    # no valid route: two chains of one layer; gc > breakage: the same, by another cause
    choice, cs, covs = _tiny([bad] * 4, [[3, 1], [5, 1]])
    assert choice.tolist() == [1, 1] and cs.tolist() == [1, 1] and covs[0]["starts"]["no_transition"] == 1
    choice, cs, covs = _tiny([1000] * 4, [[3, 1], [5, 1]], brk=9.0)
    assert cs.tolist() == [1, 1] and covs[0]["starts"]["breakage"] == 1
    choice, cs, covs = _tiny([1000] * 4, [[3, 1], [5, 1]], brk=10.0)   # gc == breakage chains on
    assert cs.tolist() == [1, 0]


# ---- the sets

@pytest.mark.parametrize("name", vs.NAMES)
def test_reference_equals_oracle(dense, name):
    c = covered(dense, name)
    tr = c["set"]["tr"]
    vr.assert_equal(c["ref"]["choice"], c["ref"]["chain_start"], c["choice"], c["cs"], c["covs"], tr["trace_off"],
                    c["ref"]["n_states"], name + ": oracle against viterbi_ref")
    assert int(c["ref"]["n_states"].sum()) == c["tot"]["layers"] > 0


def test_mixed_reaches_every_layer_shape(dense):
    plain, turns = covered(dense, "mixed")["tot"], covered(dense, "mixed_turns")["tot"]
    for tot in (plain, turns):
        assert tot["cells"].min() >= 10, tot["cells"]
        assert tot["starts"]["empty"] >= 20
        assert tot["starts"]["no_transition"] >= 3
        assert tot["no_transition_ka"][0] >= 1      # the K_A <= 4 pass of k_viterbi_w falls through on its own
        assert tot["starts"]["breakage"] >= 50
        assert tot["cut_wave"] >= 20 and tot["cut_batch"] >= 20
        assert tot["k16_layers"] >= 50
    assert plain["source_ties"] >= 20 and turns["source_ties"] >= 5
    assert plain["winner_ties"] >= 1
    # trace 3 stands still for four points and keeps them as states: layers with gc = 0
    c = covered(dense, "mixed")
    o = int(c["set"]["tr"]["trace_off"][3])
    assert c["ref"]["n_states"][3] == 90 and (c["ref"]["gc"][o + 41:o + 44] == 0.0).all()


@pytest.mark.parametrize("name,chains", [("long4", 3), ("long6", 4)])
def test_long_has_chains_past_a_backtrace_block(dense, name, chains):
    tot = covered(dense, name)["tot"]
    assert sum(tot["long_chains"].values()) >= chains, tot["long_chains"]
    for why in ("empty", "breakage", "end"):
        assert tot["long_chains"][why] >= 1, tot["long_chains"]
    assert tot["single_wave"] >= 400 and tot["single_batch"] >= 400
    # the breakage break has candidates on both sides; one layer has gc == breakage_distance and chains on
    assert tot["starts"]["breakage"] == 1 and tot["starts"]["empty"] == 1
    assert tot["gc_at_breakage"] >= 1


@pytest.mark.parametrize("name", ["many", "many_turns", "empty"])
def test_many_mixes_traces_in_a_wave(dense, name):
    c = covered(dense, name)
    tot, ns = c["tot"], c["ref"]["n_states"].astype(np.int64)
    assert tot["cells"].min() >= 10, tot["cells"]
    assert tot["starts"]["no_transition"] >= 50
    if name != "many_turns":     # (turn costs break most ties: the plain runs carry these)
        assert tot["source_ties"] >= 200 and tot["winner_ties"] >= 10
    T = len(ns)
    assert T == vs.MANY_T and T % 4 == 1
    groups = [g for g in range(0, T - 3, 4) if ns[g:g + 4].min() >= 20 and len(set(ns[g:g + 4].tolist())) == 4]
    assert len(groups) >= 3, groups
    # a hot trace in each group position among fillers, one cut to a single point, one alone in the last wave
    assert {k % 4 for k in vs.MANY_HOT if ns[k] >= 20 and (ns[k - k % 4:k - k % 4 + 4] >= 20).sum() == 1} == {0, 1, 2, 3}
    assert ns[3] == 1 and ns[T - 1] >= 20
    lengths = np.diff(c["set"]["tr"]["trace_off"].astype(np.int64))
    assert (int((lengths == 0).sum()) >= 500) == (name == "empty")


@pytest.mark.parametrize("name", ["small_four", "small_four_turns"])
def test_small_four_is_one_wave_of_everything(dense, name):
    c = covered(dense, name)
    tot = c["tot"]
    assert np.diff(c["set"]["tr"]["trace_off"].astype(np.int64)).tolist() == [90, 37, 64, 5]
    assert tot["cells"].min() >= 1, tot["cells"]
    assert tot["starts"]["empty"] >= 1
    assert tot["source_ties"] + tot["winner_ties"] >= 1
