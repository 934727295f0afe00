"""Rule 20 without a GPU: the plain-Python reference (inflate_ref.py) equals Python's zlib and gzip
on the catalogue of deflate_make.py, the host decoder (engine.inflate_host: the core of
reporter_amd/csrc/inflate_core.hpp on the host pool) equals both status for status, and the
catalogue reaches what it claims to reach (the reference's counts).  The tests that check the
reference and the catalogue themselves against zlib and gzip (test_reference_*, test_catalogue_*,
test_header_extra_fields, test_sizes_are_what_they_claim) need no decoder of the library's, so
unlike the rest they do not depend on the library's entry points."""
import gzip
import zlib

import pytest

import deflate_make as dm
import inflate_ref as ir
from reporter_amd import engine


def _zlib_members(z):
    """z's members through zlib's own inflate (wbits 31), zero padding skipped"""
    out = []
    while z:
        d = zlib.decompressobj(31)
        out.append(d.decompress(z))
        assert d.eof
        z = d.unused_data.lstrip(b"\0")
    return b"".join(out)


@pytest.fixture(scope="module")
def ref():
    """name -> (chunk, bytes, status, counts) over the three catalogues, and the counts summed"""
    total = ir.new_counts()
    out = {}
    for name, z in dm.catalogue() + dm.size_catalogue():
        b, s, k = ir.inflate(z)
        out[name] = (z, b, s, k)
        for key, v in k.items():
            total[key] = (total[key] | v) if key == "flags_seen" else max(total[key], v) if key.startswith("max_") else total[key] + v
    for name, z, _ in dm.error_catalogue():
        out[name] = (z,) + ir.inflate(z)
    return out, total


def test_reference_equals_zlib(ref):
    for name, z in dm.catalogue() + dm.size_catalogue():
        _, b, s, _ = ref[0][name]
        assert s == ir.OK, name
        assert b == gzip.decompress(z), name
        if name != "all_flags":   # (zlib's own header reader refuses reserved flag bits and a wrong FHCRC: rule 20's two deviations)
            assert b == _zlib_members(z), name
        if name not in ("three_members", "padded", "all_flags", "nothing"):
            assert b == zlib.decompress(z, 31), name


def test_reference_statuses(ref):
    for name, z, status in dm.error_catalogue():
        assert ref[0][name][2] == status, name
        assert ref[0][name][1] is None
        with pytest.raises((gzip.BadGzipFile, EOFError, zlib.error)) as e:   # the module the reference runs refuses it too
            gzip.decompress(z)
        kind = {1: gzip.BadGzipFile, 2: EOFError, 3: zlib.error, 4: gzip.BadGzipFile, 5: gzip.BadGzipFile}[status]
        assert e.type is kind, (name, e.type)


def test_catalogue_reaches_the_edges(ref):
    k = ref[1]
    one = {name: v[3] for name, v in ref[0].items() if len(v) == 4}
    assert k["stored"] and k["fixed"] and k["dynamic"]                                   # (a)
    assert k["max_member_dynamic"] >= 3 and one["blocks"]["max_member_dynamic"] >= 3     # (b)
    assert k["max_lit_bits"] == 15 and k["max_dist_bits"] == 15                          # (c)
    assert k["max_length"] == 258 and k["max_distance"] == 32768                         # (d)
    assert k["distance_1"] and k["overlapping"]                                          # (e)
    assert k["stored_empty"] and k["stored_max"] and k["stored_unaligned"]               # (f)
    assert k["earlier_block"] and k["ring_wrap"] and k["wrap_from_earlier_block"]        # (g)
    assert one["three_members"]["members"] == 3 and k["empty_members"] and k["one_byte_members"]   # (h)
    assert one["padded"]["padding"] == 5 + 1 + 512 and one["padded"]["members"] == 3
    assert k["flags_seen"] == 0xff
    assert k["one_code_dist"] and k["zero_dist_literals"]                                # (i)
    # what zlib's own choices give on the trace lines and the mix
    assert one["lines_l0"]["stored"] >= 4 and one["lines_l0"]["dynamic"] == 0
    assert one["lines_fixed"]["fixed"] >= 1 and one["lines_fixed"]["dynamic"] == 0
    assert one["lines_l6"]["dynamic"] >= 1
    assert one["mix"]["max_member_dynamic"] >= 3 and one["mix"]["max_length"] == 258


def test_header_extra_fields():
    """FEXTRA of 0 and of 300 bytes are both in the all_flags chunk"""
    z = dict(dm.catalogue())["all_flags"]
    assert z[3] & 4 and z[10:12] == b"\0\0"
    second = z.index(b"\x1f\x8b", 12)
    assert z[second + 3] & 4 and z[second + 10:second + 12] == (300).to_bytes(2, "little")


def test_host_decoder_equals_reference(ref):
    names = [n for n, _ in dm.catalogue() + dm.size_catalogue()]
    out, status = engine.inflate_host([ref[0][n][0] for n in names])
    for n, b, s in zip(names, out, status):
        assert s == 0, n
        assert b == ref[0][n][1], n
    info = engine.inflate_last()
    assert info["members"] == sum(ref[0][n][3]["members"] for n in names)
    assert info["bytes_out"] == sum(len(ref[0][n][1]) for n in names)


def test_host_decoder_statuses(ref):
    """every bad stream between two good ones: its status, and the good ones intact"""
    good = ref[0]["lines_l6"]
    chunks, want = [], []
    for name, z, status in dm.error_catalogue():
        chunks += [good[0], z]
        want += [0, status]
    chunks.append(good[0])
    want.append(0)
    out, status = engine.inflate_host(chunks)
    names = [n for n, _, _ in dm.error_catalogue()]
    assert status == want, [(names[i // 2], s, w) for i, (s, w) in enumerate(zip(status, want)) if s != w]
    for b, s in zip(out, status):
        assert (b == good[1]) if s == 0 else (b is None)


def test_status_text():
    texts = [engine.inflate_status_text(s) for s in range(7)]
    assert texts[0] == "ok" and len(set(texts)) == 7
    assert "CRC" in texts[4]


def test_sizes_are_what_they_claim():
    sizes = dict(dm.size_catalogue())
    for n in (0, 1, 16383, 16384, 16385, 32767, 32768, 32769, 65537):
        assert len(gzip.decompress(sizes["out_%d" % n])) == n
    for n in (1023, 1024, 1025):
        assert len(sizes["in_%d" % n]) == n
