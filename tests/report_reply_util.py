"""Shared by the /report reply tests (DESIGN.md §3 rule 19): the reference's 415 report() cases as
segment, report and stats records, and what a parsed reply must equal."""
import json
import os

import numpy as np

from reporter_amd import engine

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "report_golden.json")
INVALID = engine.INVALID_SEGMENT_ID


def segment_records(segs):
    """SEGMENT_DTYPE records of reply-schema segment dicts, way ids from ``way_ids``."""
    a = np.zeros(len(segs), engine.SEGMENT_DTYPE)
    for i, s in enumerate(segs):
        has = s.get("segment_id") is not None
        a[i]["segment_id"] = s["segment_id"] if has else INVALID
        a[i]["start_time"] = s["start_time"]
        a[i]["end_time"] = s["end_time"]
        a[i]["length"] = s["length"]
        a[i]["queue_length"] = s["queue_length"]
        a[i]["flags"] = (1 if s.get("internal", False) else 0) | (2 if has else 0)
        a[i]["begin_shape_index"] = s["begin_shape_index"]
        a[i]["end_shape_index"] = s["end_shape_index"]
        a[i]["seg_dense"] = 0xFFFFFFFF
        a[i]["way_first"] = s["way_ids"][0]
        a[i]["way_last"] = s["way_ids"][-1]
    return a


def report_records(reports):
    a = np.zeros(len(reports), engine.REPORT_DTYPE)
    for i, r in enumerate(reports):
        a[i]["id"] = r["id"]
        a[i]["next_id"] = r.get("next_id", INVALID)
        a[i]["t0"], a[i]["t1"] = r["t0"], r["t1"]
        a[i]["length"], a[i]["queue_length"] = r["length"], r["queue_length"]
        a[i]["seg_dense"] = 0xFFFFFFFF
    return a


def _metres(km):
    """The metres behind a stats length: 0 stands for never assigned (no golden assigns 0 m)."""
    return -1 if km == 0 else int(round(km * 1000))


def stats_record(out):
    a = np.zeros(1, engine.STATS_DTYPE)
    st = out["stats"]
    a[0]["successful_count"] = st["successful_matches"]["count"]
    a[0]["unreported_count"] = st["unreported_matches"]["count"]
    a[0]["successful_length_m"] = _metres(st["successful_matches"]["length"])
    a[0]["unreported_length_m"] = _metres(st["unreported_matches"]["length"])
    a[0]["discontinuities"] = st["match_errors"]["discontinuities"]
    a[0]["invalid_speeds"] = st["match_errors"]["invalid_speeds"]
    a[0]["invalid_times"] = st["match_errors"]["invalid_times"]
    a[0]["unassociated"] = st["unassociated_segments"]
    a[0]["shape_used"] = out.get("shape_used", -1)
    a[0]["n_reports"] = len(out["datastore"]["reports"])
    return a


def offsets(parts):
    return np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint32)


def cat(parts, dtype):
    parts = [p for p in parts if len(p)]
    return np.concatenate(parts) if parts else np.zeros(0, dtype)


_cases = None


def golden_cases():
    global _cases
    if _cases is None:
        with open(GOLDEN) as f:
            _cases = json.load(f)["cases"]
        assert len(_cases) == 415
    return _cases


def check_reply(text, segs, want, what=""):
    """A reply's stats, shape_used and datastore equal ``want``'s, its segments the records'."""
    got = json.loads(text)
    assert list(got) == [k for k in ("stats", "shape_used", "segment_matcher", "datastore") if k != "shape_used" or "shape_used" in want], what
    assert got["stats"] == want["stats"], what
    assert got.get("shape_used") == want.get("shape_used"), what
    assert got["datastore"] == want["datastore"], what
    assert list(got["segment_matcher"]) == ["segments", "mode"] and got["segment_matcher"]["mode"] == "auto", what
    assert got["segment_matcher"]["segments"] == engine.segment_dicts(segs), what
    return got
