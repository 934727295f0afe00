"""The sections a sharded stream's snapshot adds (DESIGN.md §3 rule 17; snapshot.hpp kinds 11, 12)
on the host: tests/cpp/snapshot_shard_test.cpp on the header's own functions (built with
AddressSanitizer and UBSan where their runtimes are installed, and run directly), and the same
through rm_snapshot_check_host_shard / engine.snapshot_info with blobs laid out by
tests/snapshot_shard_ref.py's writer."""
import os
import subprocess

import numpy as np
import pytest

import snapshot_ref as sn
import snapshot_shard_ref as sh
from reporter_amd import _lib, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_snapshot_shard_cpp(tmp_path):
    exe = str(tmp_path / "snapshot_shard_test")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
            "-I" + os.path.join(ROOT, "reporter_amd", "csrc"),
            os.path.join(ROOT, "tests", "cpp", "snapshot_shard_test.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:   # no sanitizer runtime here
        subprocess.run(base, check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "snapshot shard ok" in r.stdout


def _sections(keys=(5, (1 << 32) | 2), shard=(1, 3, 4, 0)):
    meta = np.zeros(1, sn.META_DTYPE)
    meta["arrivals"], meta["quantisation"] = 9, 60
    return {sn.USER: b"hi", sn.TILE_ROWS: bytes(range(128)), sn.TILE_META: meta.tobytes(),
            sh.TILE_KEYS: np.array(keys, "<u8").tobytes(), sh.SHARD_REC: np.array(shard, "<u4").tobytes()}


def _refused(blob):
    with pytest.raises(_lib.RmError) as e:
        engine.snapshot_info(blob)
    return str(e.value)


def test_info_reports_the_shard(built_lib):
    info = engine.snapshot_info(sh.write(_sections()))
    assert (info["rank"], info["nranks"], info["calls"], info["rows"], info["user"]) == (1, 3, 4, 2, b"hi")
    plain = _sections()
    del plain[sh.TILE_KEYS], plain[sh.SHARD_REC]
    assert "nranks" not in engine.snapshot_info(sh.write(plain))   # today's blob, today's answer


def test_each_new_clause_has_its_message(built_lib):
    cases = [
        (_sections(keys=(5,)), "snapshot: the tile keys' count is not the row count"),
        (_sections(keys=(5, (1 << 64) - 1)), "snapshot: a tile row's key is the padding key"),
        (_sections(shard=(3, 3, 4, 0)), "snapshot: the shard record's rank is not below its nranks"),
        (_sections(shard=(1, 17, 4, 0)), "snapshot: the shard record's nranks is 0 or above 16"),
        (_sections(shard=(1, 3, 4, 1)), "snapshot: the shard record's padding is not zero"),
    ]
    for secs, want in cases:
        assert _refused(sh.write(secs)) == want
    s = _sections()
    del s[sh.SHARD_REC]
    assert _refused(sh.write(s)) == "snapshot: tile keys without a shard record"
    s = _sections()
    del s[sh.TILE_KEYS]
    assert _refused(sh.write(s)) == "snapshot: a shard record without tile keys"
    good = sh.write(_sections())
    _, table = sn.read(good)
    off = next(e[2] for e in table if e[0] == sh.TILE_KEYS)
    b = bytearray(good)
    b[off + 3] ^= 0x10
    assert _refused(bytes(b)) == "snapshot: a section's checksum does not match"
