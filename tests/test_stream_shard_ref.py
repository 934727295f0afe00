"""The stream on several ranks (DESIGN.md §3 rule 16) on the CPU: the two owner functions against
their Python restatement, the balance the vehicle hash must give, and the sharded model of
tests/stream_shard_ref.py against the one-rank models -- equal with the exchange, not without."""
import numpy as np
import pytest

import stream_shard_ref as ss


def test_owner_functions_are_their_restatement(built_lib):
    from reporter_amd import engine
    rng = np.random.default_rng(5)
    idx = np.concatenate([np.arange(3000), rng.integers(0, 1 << 32, 3000), [(1 << 32) - 1]])
    for R in (1, 2, 3, 8, 16):
        for i in idx.tolist():
            assert engine.vehicle_owner(i, R) == ss.vehicle_owner(i, R) < R
    buckets = np.concatenate([np.arange(200), rng.integers(0, 1 << 47, 2000)])
    tiles = rng.integers(0, 1 << 25, len(buckets))
    for R in (1, 2, 3, 8):
        for b, t in zip(buckets.tolist(), tiles.tolist()):
            assert engine.tile_file_owner(b, t, R) == ss.tile_file_owner(b, t, R) < R


@pytest.mark.parametrize("R", [2, 3, 8])
def test_vehicle_hash_balances_first_seen_order(R):
    """A condition on the hash: of the first 100,000 indices every rank gets 0.9 / R to 1.1 / R."""
    n = 100000
    own = ((np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B1) & np.uint64(ss.MASK32)) * np.uint64(R)) >> np.uint64(32)
    assert own[:1000].tolist() == [ss.vehicle_owner(i, R) for i in range(1000)]
    share = np.bincount(own.astype(np.int64), minlength=R) / n
    print("shares", R, share.min() * R, share.max() * R)
    assert share.min() >= 0.9 / R and share.max() <= 1.1 / R


@pytest.mark.parametrize("R", [2, 3])
def test_sharded_model_gives_the_one_rank_files(small_world, R):
    m = ss.models(small_world)
    one = m["one"]
    files, model = m[R]
    assert sum(len(f) for f in one) > 0 and len(one) == 3
    for want, per_rank in zip(one, files):
        union = {}
        for f in per_rank:
            assert not set(f) & set(union)
            union.update(f)
        assert union == dict(want)
    sc = ss.scenario(small_world)
    assert sum(rk.own for rk in model.ranks) == len(sc["arr"]["vehicle"])


@pytest.mark.parametrize("R", [2, 3])
def test_without_the_exchange_the_model_loses_rows(small_world, R):
    """What keeps the input honest: ranks that cull apart drop what the one-rank stream keeps."""
    sc = ss.scenario(small_world)
    one = ss.models(small_world)["one"]
    apart = ss.drive(ss.ShardedStream(R, sc["n_vehicles"], sc["match_fn"], ss.PARAMS, ss.Q, ss.PRIVACY), sc, exchange=False)
    differs = 0
    for want, per_rank in zip(one, apart):
        union = {}
        for f in per_rank:
            union.update(f)
        differs += union != dict(want)
    assert differs >= 2


@pytest.mark.parametrize("R", [2, 3])
def test_the_shared_stream_contains_every_case(small_world, R):
    """What tests/test_gpu_stream_shard.py needs of its input, found in the sharded model."""
    files, model = ss.models(small_world)[R]
    c = ss.cases(files, model)
    assert all(c[k] > 0 for k in ("run_needs_two_ranks", "double_trigger", "punctuate_rows", "segment_two_owners",
                                  "rank_without_file", "rank_without_rows")), c
    assert c["largest_exchange"] > 1024, c
