"""The two layout scans at their block, group and path edges, GPU.

Every run lays out its transitions / K2 sources and its traversal records by a block-wise exclusive
scan of per-slot counts.  One pair of apply kernels serves the three run paths (engine.hip
k_trans_apply / k_path_apply), which differ only in where a block's base comes from: scanned
partials on an ordinary run, a fold of the partials before the block on a small run, coarse buckets
of 64 blocks plus the partials inside the group on a steady run.  Each shape below is the smallest
batch at which one of those mechanisms can go wrong, and runs on all three paths of one matcher:
small (or ordinary, past the small limit), ordinary, steady.  Every run must equal the oracle at
every stage, and the three runs' segments must be the same bytes.
"""
import numpy as np
import pytest

import meili_oracle as mo
from parity_util import compare_all
from reporter_amd import engine, graphfile, world

pytestmark = pytest.mark.gpu

SMALL_LIMIT = 65_536   # engine.hip small_batch_points()

SHAPES = [
    255, 256, 257,             # the 256-slot block of the transitions' pass
    1023, 1024, 1025, 1027,    # the 1024-slot block of the records' pass, and the four-per-lane load's three-slot tail
    16_384, 16_385,            # transitions: exactly one bucket group of 64 blocks, then a second group of one slot
    65_536,                    # the largest small run: 256 partials, one per lane of the fold; one group of record blocks
    65_537,                    # records: the second bucket group (past the small limit)
]

_cache = {}


@pytest.fixture(scope="module")
def shared_engine(built_lib, small_world):
    eng = engine.Engine(small_world, 0)
    yield eng
    eng.close()


def _case(path, P):
    """A batch of exactly P points (k traces of 60 points and one of 2..61), its full-length trace
    count and the oracle's answer; computed once per shape."""
    if P not in _cache:
        k = (P - 2) // 60
        r = P - 60 * k
        assert 2 <= r <= 61
        tr = world.concat_traces(
            world.generate_traces(path, n_traces=k, n_points=60, rate_s=1.0, noise_m=5.0, seed=521),
            world.generate_traces(path, n_traces=1, n_points=r, rate_s=1.0, noise_m=5.0, seed=522))
        assert int(tr["trace_off"][-1]) == P and len(tr["trace_off"]) == k + 2
        opts = engine.default_options(1)
        ref = mo.match(graphfile.load(path), mo.Batch(tr["trace_off"], tr["lon"], tr["lat"], tr["time"], tr["accuracy"],
                                                      opts, np.zeros(k + 1, np.uint32)))
        _cache[P] = (tr, k, opts, ref)
    return _cache[P]


def _three_runs(eng, case, monkeypatch, locality=None):
    """One fresh matcher, three runs: the default environment, then RM_SMALL_BATCH_POINTS=0 twice.
    Returns the steady counter after each run."""
    tr, k, opts, ref = case
    bm = engine.BatchMatcher(eng)
    if locality is not None:
        bm.set_locality(locality)
    outs, steady = [], []
    for limit in (None, "0", "0"):
        if limit is None:
            monkeypatch.delenv("RM_SMALL_BATCH_POINTS", raising=False)
        else:
            monkeypatch.setenv("RM_SMALL_BATCH_POINTS", limit)
        bm.run(tr["trace_off"], tr["lon"], tr["lat"], tr["time"], tr["accuracy"], opts)
        c = compare_all(bm, ref, tr["trace_off"])
        assert c["transitions"] > 0 and c["segments"] > k, c
        off, segs = bm.segments()
        outs.append((off.tobytes(), segs.tobytes()))
        st = bm.run_stats()
        assert st["steady_rerun"] == 0, st
        steady.append(st["steady"])
    assert outs[0] == outs[1] == outs[2]
    bm.close()
    return steady


@pytest.mark.parametrize("P", SHAPES)
def test_layout_scans_on_every_path(shared_engine, small_world, monkeypatch, P):
    """Small (ordinary past the small limit), ordinary and steady runs of a batch of exactly P points.
    The steady counter shows the paths taken: a small run that gated itself off and fell back would
    have left the matcher ready for a steady run, and the second run would count as one."""
    steady = _three_runs(shared_engine, _case(small_world, P), monkeypatch)
    assert steady == ([0, 0, 1] if P <= SMALL_LIMIT else [0, 1, 2]), steady


def test_permuted_source_scan_over_two_blocks(shared_engine, small_world, monkeypatch):
    """257 points with the locality order forced: the ordinary path's permuted K2 source scan over two
    blocks, the second holding one slot.  Every run stays on the ordinary path."""
    steady = _three_runs(shared_engine, _case(small_world, 257), monkeypatch, locality=2)
    assert steady == [0, 0, 0], steady
