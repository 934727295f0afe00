"""The stream snapshot on the host (DESIGN.md §3 rule 15; snapshot.hpp): tests/cpp/snapshot_test.cpp
on the header's own functions (built with AddressSanitizer and UBSan where their runtimes are
installed, and run directly), and the same through rm_snapshot_check_host with blobs laid out by
tests/snapshot_ref.py -- a blob whose checksums numpy computed is accepted, so the restatement the
GPU tests forge blobs with agrees with the library's; every truncation, every single flipped bit of
header and table and one forged blob per clause of the structural rule (checksums recomputed) is
refused with its message."""
import os
import struct
import subprocess

import numpy as np
import pytest

import snapshot_ref as sn
from reporter_amd import _lib, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_snapshot_cpp(tmp_path):
    exe = str(tmp_path / "snapshot_test")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
            "-I" + os.path.join(ROOT, "reporter_amd", "csrc"),
            os.path.join(ROOT, "tests", "cpp", "snapshot_test.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:   # no sanitizer runtime here
        subprocess.run(base, check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "snapshot ok" in r.stdout


def _sections():
    rec = np.zeros(2, sn.REC_DTYPE)
    rec["vehicle"], rec["cnt"], rec["max_sep"], rec["last_update"] = [1, 4], [2, 3], [3.5, 0.0], [1000, 2000]
    meta = np.zeros(1, sn.META_DTYPE)
    meta["arrivals"], meta["quantisation"] = 9, 60
    return {sn.USER: b"hello",
            sn.DIR_OFF: np.array([0, 3, 7, 12], "<u8").tobytes(), sn.DIR_BYTES: b"abcdefghijkl",
            sn.SESS_REC: rec.tobytes(),
            sn.SESS_LON: np.arange(5, dtype="<f4").tobytes(), sn.SESS_LAT: np.arange(5, dtype="<f4").tobytes(),
            sn.SESS_ACC: np.full(5, -1, "<f4").tobytes(), sn.SESS_TIME: np.arange(10, 15, dtype="<f8").tobytes(),
            sn.TILE_ROWS: bytes(range(128)), sn.TILE_META: meta.tobytes()}


def _refused(blob):
    with pytest.raises(_lib.RmError) as e:
        engine.snapshot_info(blob)
    assert str(e.value).startswith("snapshot: "), str(e.value)
    return str(e.value)


def test_numpy_blob_is_accepted(built_lib):
    blob = sn.write(_sections())
    info = engine.snapshot_info(blob)
    assert info == dict(version=1, bytes=len(blob), names=3, vehicles=2, points=5, rows=2, quantisation=60,
                        user_offset=info["user_offset"], user_bytes=5, user=b"hello")
    assert len(blob) % 16 == 0 and info["user_offset"] % 16 == 0
    secs, table = sn.read(blob)
    assert secs == _sections() and all(sn.checksum(secs[e[0]]) == e[5] for e in table)
    assert engine.snapshot_info(sn.write({}))["bytes"] == 32
    # the checksum changes under any single flipped bit (every bit of one word, one bit of every word)
    data = bytearray(os.urandom(4096))
    base = sn.checksum(data)
    for bit in list(range(64)) + list(range(64, 4096 * 8, 61)):
        data[bit // 8] ^= 1 << (bit % 8)
        assert sn.checksum(data) != base
        data[bit // 8] ^= 1 << (bit % 8)


def test_truncations_and_flipped_bits_are_refused(built_lib):
    blob = sn.write(_sections())
    for n in range(len(blob)):
        _refused(blob[:n])
    d0 = sn.align16(32 + 40 * len(_sections()))
    seen = set()
    for bit in range(d0 * 8):
        b = bytearray(blob)
        b[bit // 8] ^= 1 << (bit % 8)
        seen.add(_refused(bytes(b)))
    assert {"snapshot: bad magic", "snapshot: unknown format version", "snapshot: its length differs from the header's",
            "snapshot: the checksum of header and table does not match"} <= seen
    for bit in range(d0 * 8, len(blob) * 8, 7):   # behind them: a section's checksum, or its padding
        b = bytearray(blob)
        b[bit // 8] ^= 1 << (bit % 8)
        assert _refused(bytes(b)) in ("snapshot: a section's checksum does not match", "snapshot: padding is not zero")


def _entry(table, kind):
    return next(e for e in table if e[0] == kind)


def _edit(kind, field, value):
    def f(table):
        e = _entry(table, kind)
        e[field] = value(e, table) if callable(value) else value
    return f


KIND, ELEM, OFF, BYTES, COUNT = range(5)


def test_forged_blobs_are_refused_clause_by_clause(built_lib):
    good = sn.write(_sections())
    total = len(good)
    table_cases = [
        (sn.retable(good, lambda t: None, header={"version": 2}), "snapshot: unknown format version"),
        (sn.retable(good, _edit(sn.USER, KIND, 77)), "snapshot: unknown section kind"),
        (sn.retable(good, _edit(sn.SESS_LAT, KIND, sn.SESS_LON)), "snapshot: a section kind appears twice"),
        (sn.retable(good, _edit(sn.DIR_BYTES, OFF, lambda e, t: e[OFF] + 8)), "snapshot: a section is misaligned"),
        (sn.retable(good, _edit(sn.TILE_META, OFF, total)), "snapshot: a section runs past the end"),
        (sn.retable(good, _edit(sn.DIR_BYTES, OFF, lambda e, t: _entry(t, sn.DIR_OFF)[OFF])), "snapshot: sections overlap"),
        (sn.retable(good, _edit(sn.SESS_REC, COUNT, 3)), "snapshot: a section's count times size is not its bytes"),
    ]
    for blob, want in table_cases:
        assert _refused(blob) == want

    def forged(**kw):
        s = _sections()
        rec = np.frombuffer(s[sn.SESS_REC], sn.REC_DTYPE).copy()
        off = np.frombuffer(s[sn.DIR_OFF], "<u8").copy()
        time = np.frombuffer(s[sn.SESS_TIME], "<f8").copy()
        for k, v in kw.items():
            if k == "names":
                s[sn.DIR_BYTES] = v
            elif k == "off":
                off = np.array(v, "<u8")
            elif k == "time":
                time[v[0]] = v[1]
            else:
                rec[k][v[0]] = v[1]
        s[sn.SESS_REC], s[sn.DIR_OFF], s[sn.SESS_TIME] = rec.tobytes(), off.tobytes(), time.tobytes()
        return sn.write(s)

    cases = [
        (forged(vehicle=(1, 1)), "snapshot: session vehicle indices are not strictly increasing"),
        (forged(cnt=(0, 0)), "snapshot: a session record has a cnt of 0"),
        (forged(cnt=(1, 4)), "snapshot: the session records' cnt do not add up to the point count"),
        (forged(max_sep=(0, -1.0)), "snapshot: a session max_sep is negative or not finite"),
        (forged(max_sep=(1, np.inf)), "snapshot: a session max_sep is negative or not finite"),
        (forged(time=(2, np.nan)), "snapshot: a point time is NaN"),
        (forged(off=[0, 8, 7, 12]), "snapshot: name offsets are not monotone"),
        (forged(off=[0, 3, 7, 20]), "snapshot: name offsets do not stay inside the name bytes"),
        (forged(off=[0, 0, 7, 12]), "snapshot: a name is empty or longer than 4096 bytes"),
        (forged(off=[0, 3, 9, 9 + 4097], names=b"abcdefghi" + b"x" * 4097), "snapshot: a name is empty or longer than 4096 bytes"),
        (forged(off=[0, 3, 7, 10], names=b"abcdefgabc"), "snapshot: two names are equal"),
    ]
    for blob, want in cases:
        assert _refused(blob) == want
    s = _sections()
    del s[sn.SESS_TIME]
    assert _refused(sn.write(s)) == "snapshot: the session sections are incomplete"
    assert struct.unpack_from("<I", good, 8)[0] == 1
