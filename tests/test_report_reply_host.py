"""The /report reply on the host (DESIGN.md §3 rule 19), no GPU.

1. The reference's 415 report() cases (tests/golden/report_golden.json) as segment, report and
   stats records through rm_report_format_host: every parsed reply has the golden's stats,
   shape_used and datastore -- the reference's own results -- and the records' segments.
2. The request reader's level arrays (tests/cpp/report_levels_test.cpp, which includes
   trace_json.hpp as tests/cpp/trace_json_test.cpp does): masks as engine.levels_mask gives them,
   the first match_options wins, the service's texts for a missing or non-array value, the stated
   text for a non-number entry, and Match's own reading of the same requests unchanged.
"""
import json
import os
import subprocess

import numpy as np

from reporter_amd import engine
import report_reply_util as ru

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_replies_equal_reference_goldens(built_lib):
    cases = ru.golden_cases()
    segs = [ru.segment_records(c["input"]["match"]["segments"]) for c in cases]
    reps = [ru.report_records(c["output"]["datastore"]["reports"]) for c in cases]
    stats = np.concatenate([ru.stats_record(c["output"]) for c in cases])
    replies = engine.format_replies_host(ru.offsets(segs), ru.cat(segs, engine.SEGMENT_DTYPE), ru.offsets(reps),
                                         ru.cat(reps, engine.REPORT_DTYPE), stats)
    assert len(replies) == 415
    n_rep = n_shape = 0
    for i, (c, text) in enumerate(zip(cases, replies)):
        got = ru.check_reply(text, segs[i], c["output"], "case %d" % i)
        n_rep += len(got["datastore"]["reports"])
        n_shape += "shape_used" in got
        assert b" " not in text and b"\n" not in text   # compact separators
    assert n_rep > 150 and 0 < n_shape < 415


def test_host_reply_text_of_one_trace(built_lib):
    """The bytes of one reply, spelled out: key order, three fixed decimals, shortest times."""
    segs = ru.segment_records([
        {"segment_id": 234881064, "way_ids": [1, 7], "start_time": 1500000000.5, "end_time": 1500000030.25, "queue_length": 0,
         "length": 1234, "internal": False, "begin_shape_index": 0, "end_shape_index": 5},
        {"way_ids": [2], "start_time": 1500000030.25, "end_time": -1, "queue_length": 3, "length": -1, "internal": True,
         "begin_shape_index": 5, "end_shape_index": 9}])
    reps = ru.report_records([{"id": 234881064, "t0": 1500000000.5, "t1": 1500000030.25, "length": 1234, "queue_length": 0}])
    stats = np.zeros(1, engine.STATS_DTYPE)
    stats[0]["successful_count"], stats[0]["successful_length_m"], stats[0]["unreported_length_m"] = 1, 1234, -1
    stats[0]["shape_used"], stats[0]["n_reports"] = 5, 1
    (text,) = engine.format_replies_host([0, 2], segs, [0, 1], reps, stats)
    assert text == (
        b'{"stats":{"successful_matches":{"count":1,"length":1.234},"unreported_matches":{"count":0,"length":0},'
        b'"match_errors":{"discontinuities":0,"invalid_speeds":0,"invalid_times":0},"unassociated_segments":0},"shape_used":5,'
        b'"segment_matcher":{"segments":[{"segment_id":234881064,"way_ids":[1,7],"start_time":1500000000.5,'
        b'"end_time":1500000030.25,"queue_length":0,"length":1234,"internal":false,"begin_shape_index":0,"end_shape_index":5},'
        b'{"way_ids":[2],"start_time":1500000030.25,"end_time":-1,"queue_length":3,"length":-1,"internal":true,'
        b'"begin_shape_index":5,"end_shape_index":9}],"mode":"auto"},"datastore":{"mode":"auto","reports":['
        b'{"id":234881064,"t0":1500000000.5,"t1":1500000030.25,"length":1234,"queue_length":0}]}}')
    # a time outside the routine's range: the trace is written with std::to_chars instead
    segs[1]["start_time"] = 0.5
    segs[0]["end_time"] = 1e300
    (text,) = engine.format_replies_host([0, 2], segs, [0, 1], reps, stats)
    got = json.loads(text)["segment_matcher"]["segments"]
    assert got[1]["start_time"] == 0.5 and got[0]["end_time"] == 1e300 and b'"end_time":1e+300' in text
    # no traces: an empty buffer
    assert engine.format_replies_host([0], segs[:0], [0], reps[:0], stats[:0]) == []


def test_request_level_arrays(tmp_path):
    exe = str(tmp_path / "report_levels_test")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
            "-I" + os.path.join(ROOT, "reporter_amd", "csrc"),
            os.path.join(ROOT, "tests", "cpp", "report_levels_test.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    sanitized = subprocess.run(base + san, capture_output=True).returncode == 0
    if not sanitized:   # no sanitizer runtime here (a real compile error fails this build too)
        subprocess.run(base, check=True)
    print("report_levels_test built %s" % ("with ASan and UBSan" if sanitized else "without sanitizers"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "report levels ok" in r.stdout
