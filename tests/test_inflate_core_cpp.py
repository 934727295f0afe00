"""The decoder core k_inflate runs (reporter_amd/csrc/inflate_core.hpp) as a host program under
AddressSanitizer and UBSan (tests/cpp/inflate_core_test.cpp): the whole catalogue of
deflate_make.py with its expected statuses and bytes, then 24,000 byte- and bit-mutated copies,
each of which must end with a status and nothing for the sanitizers to report.  The GPU is given
the named catalogue only; the mutations run here."""
import os
import struct
import subprocess
import zlib

import deflate_make as dm
import inflate_ref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_inflate_core(tmp_path):
    rows = [(z, 0) for _, z in dm.catalogue() + dm.size_catalogue()] + [(z, s) for _, z, s in dm.error_catalogue()]
    blob = [struct.pack("<I", len(rows))]
    for z, status in rows:
        b, s, _ = ir.inflate(z)
        assert s == status
        blob.append(struct.pack("<I", len(z)) + z + struct.pack("<III", status, len(b or b""), zlib.crc32(b or b"") if b is not None else 0))
    cat = tmp_path / "catalogue.bin"
    cat.write_bytes(b"".join(blob))
    exe = str(tmp_path / "inflate_core_test")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
            "-I" + os.path.join(ROOT, "reporter_amd", "csrc"),
            os.path.join(ROOT, "tests", "cpp", "inflate_core_test.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    # the sanitizers are dropped only where a one-line program cannot be built with them either (no
    # runtime installed); where it can, this program must build with them too
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    have = subprocess.run(["g++", str(probe), "-o", str(tmp_path / "probe")] + san, capture_output=True).returncode == 0
    b = subprocess.run(base + (san if have else []), capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    print("inflate_core_test built %s the sanitizers" % ("with" if have else "WITHOUT"))
    r = subprocess.run([exe, str(cat), "24000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "inflate core ok" in r.stdout and "24000 mutated runs" in r.stdout
