"""The matched-edges reply formatter and polyline encoder (edges_json.hpp) on the host: the
published precision-5 vector, a round trip at 1e6 through a decoder written for the test, negative
and zero differences, an empty shape, and an edge entry with every optional key absent and present
(tests/cpp/edges_json_test.cpp).  The program is built with AddressSanitizer and UBSan where their
runtimes are installed, and run directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_edges_json(tmp_path):
    exe = str(tmp_path / "edges_json_test")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
            "-I" + os.path.join(ROOT, "reporter_amd", "csrc"),
            os.path.join(ROOT, "tests", "cpp", "edges_json_test.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:   # no sanitizer runtime here
        subprocess.run(base, check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "edges json ok" in r.stdout
