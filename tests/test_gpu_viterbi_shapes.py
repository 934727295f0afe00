"""K3's two kernels at every layer shape, GPU.

launch_viterbi picks the kernel by the trace count alone: k_viterbi_w (a wave per trace) for 5 to
4,096 traces, k_viterbi (four traces per wave) otherwise.  The sets of tests/viterbi_sets.py have
4, 4, 6, 12 and 4,101 traces, and tests/test_viterbi_ref.py asserts on the CPU which branches of
either kernel each set reaches.  Every run here is compared twice, both times for exact equality:

* every stage with the oracle (parity_util.compare_all);
* K3 alone: tests/viterbi_ref.py, run on the engine's own candidates, routes and distance terms,
  against the engine's choice and chain_start.  This reference shares only the specification with
  the oracle and the kernels, and it reads what K3 read, so a K3 defect cannot hide behind an equal
  one elsewhere.

The kernel bounds can be moved by RM_VIT_WAVE_MIN / RM_VIT_WAVE_MAX, which launch_viterbi reads
once per process: the tests require both unset instead of setting them."""
import os

import numpy as np
import pytest

import meili_oracle as mo
import viterbi_ref as vr
import viterbi_sets as vs
from parity_util import compare_all
from reporter_amd import engine, graphfile

pytestmark = pytest.mark.gpu

WAVE_MIN, WAVE_MAX = 5, 4096      # engine.hip RM_VIT_WAVE_MIN / RM_VIT_WAVE_MAX


def kernel_for(T):
    return "k_viterbi_w" if WAVE_MIN <= T <= WAVE_MAX else "k_viterbi"


@pytest.fixture(scope="module")
def site(built_lib, tmp_path_factory):
    """The dense world, one engine, and every set with its oracle outputs (built once)."""
    path = vs.dense_world(str(tmp_path_factory.mktemp("vitgpu") / "dense.rmg"))
    g = graphfile.load(path)
    eng = engine.Engine(path, 0)
    cache = {}

    def get(name):
        if name not in cache:
            s = vs.build(name, path)
            tr = s["tr"]
            cache[name] = (s, mo.match(g, mo.Batch(tr["trace_off"], tr["lon"], tr["lat"], tr["time"], tr["accuracy"],
                                                   s["opts"], s["topt"])))
        return cache[name]
    yield dict(eng=eng, get=get)
    eng.close()


@pytest.fixture(params=["small", "ordinary"])
def run_path(request, monkeypatch):
    """As small batches come (Matcher::run_small), or the ordinary run (RM_SMALL_BATCH_POINTS=0)."""
    if request.param == "ordinary":
        monkeypatch.setenv("RM_SMALL_BATCH_POINTS", "0")
    else:
        monkeypatch.delenv("RM_SMALL_BATCH_POINTS", raising=False)
    return request.param


def check_outputs(bm, s, ref, what):
    """Both comparisons on the matcher's last run."""
    tr = s["tr"]
    c = compare_all(bm, ref, tr["trace_off"])
    n_states, _ = bm.states()
    cand_n, _, _, cand_sq = bm.candidates()
    trans_off, gc, route = bm.routes()
    turns = bool((s["opts"]["turn_penalty_factor"] > 0).any())
    route_d = bm.route_terms()
    assert (route_d is not None) == turns
    choice, cs, covs = vr.viterbi_ref(tr["trace_off"], n_states, cand_n, cand_sq, trans_off, gc, route, route_d,
                                      s["opts"], s["topt"])
    got_choice, got_cs = bm.viterbi()
    vr.assert_equal(got_choice, got_cs, choice, cs, covs, tr["trace_off"], n_states, what)
    tot = vr.total(covs)
    assert tot["layers"] == c["states"] > 0
    print("K3 shapes", what, c, vr.summary(tot))
    return tot


def default_kernel_bounds():
    assert "RM_VIT_WAVE_MIN" not in os.environ and "RM_VIT_WAVE_MAX" not in os.environ


def run_set(site, name, what, rerun=False):
    default_kernel_bounds()
    s, ref = site["get"](name)
    tr = s["tr"]
    T = len(tr["trace_off"]) - 1
    what = "%s (%d traces, %s, %s)" % (name, T, kernel_for(T), what)
    bm = engine.BatchMatcher(site["eng"])
    try:
        bm.run(tr["trace_off"], tr["lon"], tr["lat"], tr["time"], tr["accuracy"], s["opts"], s["topt"])
        tot = check_outputs(bm, s, ref, what)
        if rerun:
            before = bm.run_stats()
            bm.rerun()
            after = bm.run_stats()
            assert after["steady"] == before["steady"] + 1 and after["steady_rerun"] == before["steady_rerun"], after
            check_outputs(bm, s, ref, what + ", steady rerun")
    finally:
        bm.close()
    return T, tot


@pytest.mark.parametrize("name", ["mixed", "mixed_turns"])
def test_mixed_layers_one_wave_per_trace(site, name, run_path):
    T, tot = run_set(site, name, run_path)
    assert kernel_for(T) == "k_viterbi_w" and tot["cells"].min() >= 10


@pytest.mark.parametrize("name", ["small_four", "small_four_turns"])
def test_mixed_layers_four_traces_in_one_wave(site, name, run_path):
    T, tot = run_set(site, name, run_path)
    assert kernel_for(T) == "k_viterbi" and tot["cells"].min() >= 1


@pytest.mark.parametrize("name,kernel", [("long4", "k_viterbi"), ("long6", "k_viterbi_w")])
def test_long_chains_and_mid_chunk_ends(site, name, kernel):
    T, tot = run_set(site, name, "small")
    assert kernel_for(T) == kernel
    assert all(tot["long_chains"][why] >= 1 for why in ("empty", "breakage", "end")), tot["long_chains"]


@pytest.mark.parametrize("name", ["many", "many_turns"])
def test_many_traces_of_different_lengths_share_waves(site, name):
    T, tot = run_set(site, name, "small")
    assert kernel_for(T) == "k_viterbi" and T % 4 == 1 and tot["cells"].min() >= 10


def test_many_traces_steady_rerun(site, monkeypatch):
    monkeypatch.setenv("RM_SMALL_BATCH_POINTS", "0")
    T, _ = run_set(site, "many", "ordinary", rerun=True)
    assert kernel_for(T) == "k_viterbi"


def test_empty_traces_among_many(site):
    """Every fifth filler trace has no points.  Kept last and alone, so that it can be judged on
    its own."""
    default_kernel_bounds()
    s, _ = site["get"]("empty")
    assert int((np.diff(s["tr"]["trace_off"].astype(np.int64)) == 0).sum()) >= 500
    T, tot = run_set(site, "empty", "small")
    assert kernel_for(T) == "k_viterbi" and tot["cells"].min() >= 10
