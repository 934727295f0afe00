"""The compact and the generic reader of either kind of line under eight date patterns
(time_pattern.hpp; DESIGN.md §3 rule 18) against each other on the host over 20,000 generated
lines, half of them byte-mutated: equal values, id spans and hashes wherever the compact reader
accepts, every unmutated line accepted with the instant that was written, and no byte read outside
the line's 256 (tests/cpp/time_pattern_test.cpp).  The program is built with AddressSanitizer and
UBSan where their runtimes are installed, and run directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_time_patterns(tmp_path):
    exe = str(tmp_path / "time_pattern_test")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
            "-I" + os.path.join(ROOT, "reporter_amd", "csrc"),
            os.path.join(ROOT, "tests", "cpp", "time_pattern_test.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:   # no sanitizer runtime here
        subprocess.run(base, check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "time patterns ok" in r.stdout
