"""Rule 20 on the GPU: engine.inflate (k_inflate, a wave per chunk; k_text_gather) against Python's
zlib byte for byte on the valid catalogue of deflate_make.py, against the reference's statuses on
the error catalogue mixed with valid chunks, and at the sizes at which the kernel takes another
path: the window ring's halves and wrap, the input refill, the chunk counts around a wave's 64."""
import gzip
import zlib

import pytest

import deflate_make as dm
import inflate_ref as ir
from reporter_amd import engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def valid():
    """[(name, chunk, bytes, members)]: the expected bytes from Python's gzip, the members from the reference"""
    out = []
    for name, z in dm.catalogue() + dm.size_catalogue():
        b, s, k = ir.inflate(z)
        assert s == 0 and b == gzip.decompress(z)
        out.append((name, z, b, k["members"]))
    return out


def _second_pass(rows):
    return sum(1 for r in rows if r[3] > 1)


def test_valid_catalogue_in_one_call(valid):
    out, status = engine.inflate([z for _, z, _, _ in valid])
    info = engine.inflate_last()
    assert status == [0] * len(valid)
    for (name, z, b, _), got in zip(valid, out):
        assert got == b, name
        if name not in ("three_members", "padded", "all_flags", "nothing"):
            assert got == zlib.decompress(z, 31), name
    assert info["members"] == sum(m for _, _, _, m in valid)
    assert info["bytes_out"] == sum(len(b) for _, _, b, _ in valid)
    assert _second_pass(valid) >= 3 and info["second_pass"] == _second_pass(valid)


def test_error_catalogue_between_valid_chunks(valid):
    """every bad stream next to good ones in one call: the reference's status, the good ones byte-exact"""
    errors = dm.error_catalogue()
    chunks, want, rows = [], [], []
    for i, (name, z, status) in enumerate(errors):
        assert ir.inflate(z)[1] == status, name
        good = valid[i % len(valid)]
        chunks += [good[1], z]
        want += [(good[0], 0, good[2]), (name, status, None)]
        rows.append(good)
    out, status = engine.inflate(chunks)
    assert [(w[0], s) for w, s in zip(want, status)] == [(w[0], w[1]) for w in want]
    for w, got in zip(want, out):
        assert got == w[2], w[0]
    assert engine.inflate_last()["second_pass"] == _second_pass(rows)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
def test_chunk_counts(valid, n):
    small = [v for v in valid if len(v[2]) <= 70000]
    rows = [small[(i * 7) % len(small)] for i in range(n)]
    out, status = engine.inflate([r[1] for r in rows])
    assert status == [0] * n
    assert all(got == r[2] for got, r in zip(out, rows))
    assert engine.inflate_last()["second_pass"] == _second_pass(rows)


def test_all_empty_members():
    empty = dm.gz(b"")
    out, status = engine.inflate([empty, empty + empty, empty + b"\0" * 40, b""] * 20)
    assert status == [0] * 80 and out == [b""] * 80
    info = engine.inflate_last()
    assert info["members"] == 20 * 4 and info["bytes_out"] == 0 and info["second_pass"] == 0


def test_lying_trailers_do_not_fail_the_call(valid):
    """five chunks whose trailers promise 4 GiB each (slots are capped at 1032 bytes per input byte,
    and five times 1 MB of input still passes 2^32 together): each ends with status 5, and the
    valid chunks beside them stay byte-exact instead of the call failing as too large"""
    import random
    r = random.Random(3)
    liars = []
    for k in range(5):
        body = bytes(r.getrandbits(8) for _ in range(4096)) * 256
        liars.append(dm.gz(body, 0, isize=0xffffffff))
        assert len(liars[-1]) * 1032 > (1 << 32) // 5
    good = [v for v in valid if v[0] in ("lines_l6", "three_members", "one_byte")]
    chunks = [good[0][1]] + liars[:3] + [good[1][1]] + liars[3:] + [good[2][1]]
    out, status = engine.inflate(chunks)
    assert status == [0, 5, 5, 5, 0, 5, 5, 0]
    assert [out[0], out[4], out[7]] == [g[2] for g in good] and out[1] is None
    assert engine.inflate_last()["second_pass"] == 3
