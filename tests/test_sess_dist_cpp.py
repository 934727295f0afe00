"""The vehicle sessions' distance, float maximum and 16-wide prefix-maximum trigger search on the
host (sess_dist.hpp, shared with k_sess_trigger; tests/cpp/sess_dist_test.cpp).  The program is
built with AddressSanitizer and UBSan where their runtimes are installed, and run directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sess_dist(tmp_path):
    exe = str(tmp_path / "sess_dist_test")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
            "-I" + os.path.join(ROOT, "reporter_amd", "csrc"),
            os.path.join(ROOT, "tests", "cpp", "sess_dist_test.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:   # no sanitizer runtime here
        subprocess.run(base, check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sess dist ok" in r.stdout
