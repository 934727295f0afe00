"""The /report reply's text routines (reply_text.hpp: the time routine, kilometres with three
decimals, and the head, segment, middle, report and tail pieces) on the host, the code the kernels
of reply.hip run: over powers of two and their neighbours, every digit count, epoch-sized values
with 0..7 fractional digits and 200,000 seeded log-uniform values of [1, 2^53) the length function
equals the bytes written, the text parses back to the value with at most 17 significant digits and
not with one fractional digit fewer; every piece equals an snprintf-built expectation at the field
extremes; nothing is written outside the piece in a guarded buffer
(tests/cpp/reply_text_test.cpp).  The program is built with AddressSanitizer and UBSan where their
runtimes are installed, and run directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reply_text(tmp_path):
    exe = str(tmp_path / "reply_text_test")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
            "-I" + os.path.join(ROOT, "reporter_amd", "csrc"),
            os.path.join(ROOT, "tests", "cpp", "reply_text_test.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    sanitized = subprocess.run(base + san, capture_output=True).returncode == 0
    if not sanitized:   # no sanitizer runtime here (a real compile error fails this build too)
        subprocess.run(base, check=True)
    print("reply_text_test built %s" % ("with ASan and UBSan" if sanitized else "without sanitizers"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "reply text ok" in r.stdout
