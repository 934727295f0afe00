"""The steady scans' block bases (rm_common.hpp scan_base_lane), CPU.

A counting kernel leaves one pair of u64 partials per block, every 64 of them are summed into
one coarse bucket, and an apply block of a steady run (engine.hip k_trans_apply / k_path_apply with
BaseBuckets) forms its base from the buckets before its group and the partials before it inside
the group.  rm_scan_block_bases does exactly that on the host with the kernels'
helper, lane by lane; the bases must be the exclusive cumulative sums of the partials.  Block
counts: one block, either side of a group boundary, the GPU test's 141 and C2's 23,438.
"""
import numpy as np
import pytest


@pytest.mark.parametrize("nb", [1, 63, 64, 65, 141, 23438])
def test_block_bases_are_the_exclusive_prefix(built_lib, nb):
    from reporter_amd import _lib
    rng = np.random.default_rng(nb)
    # pairs as k_trans_count leaves them (<= 256 * 16 * 16 and <= 256 * 16 per block), a few
    # large enough to carry the sums past 2^32, and empty blocks
    part = np.stack([rng.integers(0, 65537, nb, dtype=np.uint64), rng.integers(0, 4097, nb, dtype=np.uint64)], axis=1)
    part[rng.random(nb) < 0.1] = 0
    part[rng.random(nb) < 0.02, 0] += np.uint64(1) << np.uint64(33)
    part = np.ascontiguousarray(part)
    want = np.cumsum(part, axis=0, dtype=np.uint64) - part
    for lanes in (256, 1, 7):
        got = np.full((nb, 2), 0xdeadbeef, np.uint64)
        _lib.check(_lib.lib().rm_scan_block_bases(part.ctypes.data, nb, lanes, got.ctypes.data))
        np.testing.assert_array_equal(got, want, "lanes %d" % lanes)
