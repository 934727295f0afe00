"""The keep rule of the privacy cull (tile_cull.hpp tile_run_kept) on the host, the code the
kernels of stages.hip and tilestore.hip run: every layout of up to 3 files x up to 4 runs x run
sizes 1-3 at privacy 1-3 against the reference's loop over each file's rows, among them a final
one-row run after a short run, after a long run, and a file whose only run is one row
(tests/cpp/tile_cull_test.cpp).  The program is built with AddressSanitizer and UBSan where their
runtimes are installed, and run directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tile_cull(tmp_path):
    exe = str(tmp_path / "tile_cull_test")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
            "-I" + os.path.join(ROOT, "reporter_amd", "csrc"),
            os.path.join(ROOT, "tests", "cpp", "tile_cull_test.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:   # no sanitizer runtime here
        subprocess.run(base, check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tile cull ok" in r.stdout
