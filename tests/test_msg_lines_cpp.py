"""The compact and the generic reader of JSON stream messages (msg_lines.hpp, DESIGN.md §3 rule 14)
against each other on the host over 24,000 generated lines, half of them byte-mutated: the same
status, values, id spans and hashes wherever the compact reader does not answer "host", no byte read
outside the line's 256, and every unmutated compact line taken by the compact reader
(tests/cpp/msg_lines_test.cpp).  The program is built with AddressSanitizer and UBSan where their
runtimes are installed, and run directly."""
import os
import re
import subprocess
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_msg_lines(tmp_path):
    exe = str(tmp_path / "msg_lines_test")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
            "-I" + os.path.join(ROOT, "reporter_amd", "csrc"),
            os.path.join(ROOT, "tests", "cpp", "msg_lines_test.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:   # no sanitizer runtime here
        subprocess.run(base, check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "msg lines ok" in r.stdout
    which = re.search(r"sanitizers: .*", r.stdout).group(0)
    print(which)
    if "none" in which:   # visible in pytest's summary: the out-of-bounds half was not checked
        warnings.warn("msg_lines_test ran without AddressSanitizer / UBSan: " + which)
    m = re.search(r"compact share of unmutated lines: (\d+) / (\d+)", r.stdout)
    assert m, r.stdout
    assert int(m.group(2)) >= 8000 and m.group(1) == m.group(2), r.stdout
