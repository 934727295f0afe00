"""The tile store's text routines (tile_text.hpp: digit counts, integer writers, the row, the file
name and the blob piece of a row) on the host, the code the kernels of tilestore.hip run: for every
digit count 1..19 and both edges of each, 0, 2^63 - 1, the i32 extremes and the empty next_id, the
length function equals the bytes written, the bytes equal snprintf's, and nothing is written
outside the piece in a guarded buffer (tests/cpp/tile_text_test.cpp).  The program is built with
AddressSanitizer and UBSan where their runtimes are installed, and run directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tile_text(tmp_path):
    exe = str(tmp_path / "tile_text_test")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
            "-I" + os.path.join(ROOT, "reporter_amd", "csrc"),
            os.path.join(ROOT, "tests", "cpp", "tile_text_test.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:   # no sanitizer runtime here
        subprocess.run(base, check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tile text ok" in r.stdout
