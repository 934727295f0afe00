"""The resharding model of rule 17 (tests/snapshot_shard_ref.py) held to the one-rank model, from the
models alone: the state of M ranks stopped behind a poll, dealt out to N ranks and continued, writes
the one-rank stream's files -- and the stop position the GPU tests use shows every case they need."""
import pytest

import snapshot_shard_ref as sh
import stream_shard_ref as ss


@pytest.mark.parametrize("M,N", sh.PAIRS)
def test_resharded_model_continues_as_the_one_rank_model(small_world, M, N):
    stop = sh.choose_stop(small_world)
    sc = ss.scenario(small_world)
    r = sh.resume(small_world, M, N, stop)
    c = r["cases"]
    print("stop", stop, "of", len(sc["polls"]), "polls;", M, "->", N, c)
    # there is a stop position at which every saved rank holds sessions and a saved rank holds tile rows
    assert 1 <= stop <= len(sc["polls"]) and len(r["saved"]) == M
    assert c["every_rank_has_sessions"] and c["a_rank_has_rows"]
    assert c["vehicle_changes_owner"] > 0      # a vehicle changes owner between M and N
    assert c["row_changes_holder"] > 0         # a tile row changes holder
    if M > 1:                                  # (one saved rank writes one blob)
        assert c["file_needs_two_blobs"] > 0   # a run of the next flush: rows of two saved blobs, privacy 2 only together
    # the continued files, and those before the stop, are the one-rank model's
    one = ss.models(small_world)["one"]
    got = [sh.union(f) for f in r["before"]] + [sh.union(f) for f in r["files"]]
    assert len(got) == len(one) == 3 and len(r["files"]) >= 1
    assert got == [dict(f) for f in one] and all(len(f) > 0 for f in one)
    # each file from the rank tile_file_owner names, at N ranks
    for per_rank in r["files"]:
        for rank, files in enumerate(per_rank):
            for name in files:
                span, level, index = name.split("/")
                assert ss.tile_file_owner(int(span.split("_")[0]) // ss.Q, int(level) | int(index) << 3, N) == rank
    # the loaded state: every vehicle at its owner, every row at its file's owner, rows in key order
    for rank, (recs, rows) in enumerate(r["loaded"]):
        assert all(ss.vehicle_owner(v[0], N) == rank for v in recs)
        assert all(ss.tile_file_owner(row[1], row[2], N) == rank for row in rows)
        assert [row[0] for row in rows] == sorted(row[0] for row in rows)
    assert sum(len(recs) for recs, _ in r["loaded"]) == sum(len(b["records"]) for b in r["saved"])
    assert sum(len(rows) for _, rows in r["loaded"]) == sum(len(b["rows"]) for b in r["saved"])


def test_equal_rank_counts_reshard_to_themselves(small_world):
    """M = N: every rank gets back what it saved, but for the rows of files that are not its own (they
    would have left at the next exchange)."""
    stop = sh.choose_stop(small_world)
    for M in (2, 3):
        r = sh.resume(small_world, M, M, stop)
        for rank, (recs, _) in enumerate(r["loaded"]):
            assert [v[0] for v in recs] == [v for v, _ in r["saved"][rank]["records"]]
        one = ss.models(small_world)["one"]
        assert [sh.union(f) for f in r["before"]] + [sh.union(f) for f in r["files"]] == [dict(f) for f in one]


def test_a_vehicle_in_two_blobs_is_refused(small_world):
    stop = sh.choose_stop(small_world)
    saved = [dict(b) for b in sh.stops(small_world, 2)[stop - 1][1]]
    saved[1] = dict(saved[1], records=saved[1]["records"] + saved[0]["records"][:1])
    with pytest.raises(AssertionError, match="two blobs"):
        sh.reshard(saved, 3, ss.scenario(small_world))
