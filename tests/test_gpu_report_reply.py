"""The whole /report reply from one call, written on the GPU (DESIGN.md §3 rule 19), GPU.

1. The reference's 415 report() cases through rm_report_replies: the device writer's bytes equal
   the host writer's, and the parsed replies equal the reference's own outputs.
2. Kernel edges: traces of 0, 1, 2, 63, 64, 65, 127, 128, 129 and 300 segments in an order that
   makes the writer's waves straddle traces, fields at their longest, times of 0..7 fractional
   digits; then two traces with times outside the time routine's range (flagged, spliced in).
3. End to end on the C1 world: ReportMany against report_oracle.report applied to MatchMany, with
   the reply text written on the device and on the host, per-request level sets, three thresholds.
4. Coalesced: Report and Match from eight threads give the uncoalesced bytes.
"""
import copy
import json
import threading

import numpy as np
import pytest

import report_oracle
import report_reply_util as ru
from reporter_amd import engine, world

pytestmark = pytest.mark.gpu


def _both_writers(seg_off, segs, end, thr, rmask, tmask):
    dev, di = engine.report_replies(seg_off, segs, end, thr, rmask, tmask, writer=2)
    host, hi = engine.report_replies(seg_off, segs, end, thr, rmask, tmask, writer=1)
    assert di["writer"] == 2 and hi["writer"] == 1
    assert len(dev) == len(host) == len(seg_off) - 1
    for i, (a, b) in enumerate(zip(dev, host)):
        assert a == b, "trace %d: device and host bytes differ" % i
    assert di["bytes"] == hi["bytes"] == sum(len(x) for x in dev)
    assert di["flagged"] == hi["flagged"]
    return dev, di


def test_device_replies_equal_reference_goldens(built_lib):
    cases = ru.golden_cases()
    segs = [ru.segment_records(c["input"]["match"]["segments"]) for c in cases]
    inp = [c["input"] for c in cases]
    dev, info = _both_writers(
        ru.offsets(segs), ru.cat(segs, engine.SEGMENT_DTYPE), [c["trace_end_time"] for c in inp],
        [c["threshold_sec"] for c in inp], [engine.levels_mask(c["report_levels"]) for c in inp],
        [engine.levels_mask(c["transition_levels"]) for c in inp])
    assert info["flagged"] == 0
    n_rep = 0
    for i, (c, text) in enumerate(zip(cases, dev)):
        n_rep += len(ru.check_reply(text, segs[i], c["output"], "case %d" % i)["datastore"]["reports"])
    assert n_rep > 150


# segment counts of the edge call: the empty traces first, last and adjacent; a trace's reply is
# segments + reports + 3 items, so the 64-item waves of the writer straddle every trace boundary
EDGE_COUNTS = [0, 0, 1, 63, 2, 0, 64, 65, 127, 0, 0, 128, 129, 300, 0]
FRACTIONS = [0.0, 0.5, 0.25, 0.125, 0.0625, 0.03125, 0.015625, 0.0078125]   # 0..7 fractional digits, exact in binary
LONG_ID = 0x3FFFFFFFFFF8   # 14 digits; | level 0..2


def _edge_trace(n, t):
    """n segments, each reportable with threshold 0 and levels {0,1,2} unless its length is -1:
    ten seconds and fifty metres apiece, ids and way ids at their longest (begin_shape_index below 2^31:
    ReportStats.shape_used is an int32)."""
    segs = []
    for j in range(n):
        start = 1500000000 + 1000 * t + 10 * j + FRACTIONS[(j + t) % 8]
        end = 1500000000 + 1000 * t + 10 * (j + 1) + FRACTIONS[(j + 1 + t) % 8]
        segs.append({"segment_id": LONG_ID | ((j + t) % 3), "way_ids": [0xFFFFFFFF, 0xFFFFFFFE] if j % 4 == 1 else [0xFFFFFFFF],
                     "start_time": start, "end_time": end, "queue_length": j % 7, "length": -1 if j % 11 == 5 else 50,
                     "internal": False, "begin_shape_index": 2000000000 + j, "end_shape_index": 4000000001 + j})
    return segs, 1500000000.0 + 1000 * t + 10 * n + 5


def _oracle_reply(segs, end_time, thr, levels):
    return json.loads(json.dumps(report_oracle.report({"segments": copy.deepcopy(segs)}, {"trace": [{"time": end_time}]}, thr,
                                                      set(levels), set(levels))))


def test_writer_kernel_edges(built_lib):
    traces = [_edge_trace(n, t) for t, n in enumerate(EDGE_COUNTS)]
    mask = engine.levels_mask([0, 1, 2])

    def run(traces):
        recs = [ru.segment_records(s) for s, _ in traces]
        dev, info = _both_writers(ru.offsets(recs), ru.cat(recs, engine.SEGMENT_DTYPE), [e for _, e in traces], 0.0, mask, mask)
        for i, ((s, e), text) in enumerate(zip(traces, dev)):
            want = _oracle_reply(engine.segment_dicts(recs[i]), e, 0.0, [0, 1, 2])
            assert json.loads(text) == want, "trace %d" % i
        return dev, info

    dev, info = run(traces)
    assert info["flagged"] == 0
    # every segment with a length but a trace's last is reported (a report needs the next segment)
    n_rep = sum(len(json.loads(t)["datastore"]["reports"]) for t in dev)
    assert n_rep == sum(sum(1 for q in s[:-1] if q["length"] > 0) for s, _ in traces) and n_rep > 700
    assert max(len(t) for t in dev) > 65536 and b'"reports":[]' in dev[0] and b'"segments":[]' in dev[-1]
    # two traces holding times outside the time routine's range: flagged, written on the host
    # and spliced in between the device's replies
    low, e1 = _edge_trace(5, 20)
    low[2]["start_time"] = 0.5
    high, e2 = _edge_trace(70, 21)
    high[69]["end_time"] = 1e300
    more = traces[:4] + [(low, e1)] + traces[4:9] + [(high, e2)] + traces[9:]
    dev2, info2 = run(more)
    assert info2["flagged"] == 2
    assert b'"start_time":0.5,' in dev2[4] and b'"end_time":1e+300,' in dev2[10]
    assert dev2[:4] == dev[:4] and dev2[5:10] == dev[4:9] and dev2[11:] == dev[9:]


SIZES = [2, 3, 10, 60, 61, 300]
LEVELS = [([0, 1], [0, 1]), ([0, 1, 2], [0, 1, 2]), ([], [0, 1]), ([2], []), ([0, 1], [-1, 0, 1, 2])]


@pytest.fixture(scope="module")
def service(built_lib, small_world, tmp_path_factory):
    """The C1 world configured, and 48 requests of 2, 3, 10, 60, 61 and 300 points (one point every
    five seconds, so the longer ones cross many segments), their level sets cycling."""
    import valhalla
    conf = valhalla.write_config(str(tmp_path_factory.mktemp("report") / "c1.json"), small_world, device=0, coalesce=True)
    valhalla.Configure(conf)
    sets = [world.generate_traces(small_world, 8, n, 5.0, 5.0, seed=700 + i) for i, n in enumerate(SIZES)]
    reqs, levels = [], []
    for r in range(48):
        rl, tl = LEVELS[r % 5]
        reqs.append(json.dumps(world.trace_to_request(sets[r % 6], r // 6, uuid="v%d" % r, report_levels=rl, transition_levels=tl),
                               separators=(",", ":")))
        levels.append((rl, tl))
    sm = valhalla.SegmentMatcher()
    matched = sm.MatchMany(reqs)
    yield valhalla, sm, reqs, levels, matched
    sm.close()


def test_report_many_end_to_end(service, monkeypatch):
    valhalla, sm, reqs, levels, matched = service
    n_rep = n_shape = n_noshape = n_empty = 0
    for thr in (0, 15, 60):
        monkeypatch.setenv("RM_REPLY_DEVICE_MIN_POINTS", "0")
        dev = sm.ReportMany(reqs, thr)
        info = sm.last_report_info()
        assert info["writer"] == 2 and info["flagged"] == 0 and info["bytes"] == sum(len(t.encode()) for t in dev)
        monkeypatch.setenv("RM_REPLY_DEVICE_MIN_POINTS", "1e18")
        host = sm.ReportMany(reqs, thr)
        assert sm.last_report_info()["writer"] == 1
        assert dev == host
        for i, text in enumerate(dev):
            rl, tl = levels[i]
            want = report_oracle.report(json.loads(matched[i]), json.loads(reqs[i]), thr, set(rl), set(tl))
            got = json.loads(text)
            assert got == json.loads(json.dumps(want)), (thr, i)
            n_rep += len(got["datastore"]["reports"])
            n_shape += "shape_used" in got
            n_noshape += "shape_used" not in got
            n_empty += not got["datastore"]["reports"]
    assert n_rep >= 100 and n_shape >= 1 and n_noshape >= 1 and n_empty >= 1, (n_rep, n_shape, n_noshape, n_empty)
    # Match keeps its bytes after runs with reporting on, and ignores both keys
    assert sm.MatchMany(reqs) == matched


def test_report_request_failures(service):
    valhalla, sm, reqs, levels, matched = service
    req = json.loads(reqs[3])
    for key, value, text in (("report_levels", None, "match_options must include report_levels array"),
                             ("transition_levels", None, "match_options must include transition_levels array"),
                             ("report_levels", "0,1", "match_options must include report_levels array"),
                             ("transition_levels", [0, "1"], "transition_levels entries must be numbers")):
        bad = copy.deepcopy(req)
        if value is None:
            del bad["match_options"][key]
        else:
            bad["match_options"][key] = value
        bad = json.dumps(bad, separators=(",", ":"))
        with pytest.raises(RuntimeError, match=text):
            sm.Report(bad)
        with pytest.raises(RuntimeError, match=text):
            sm.ReportMany([reqs[0], bad, reqs[1]])
        assert sm.Match(bad) == matched[3]   # Match of the same text is unaffected
    with pytest.raises(RuntimeError, match="threshold_sec must be finite"):
        sm.Report(reqs[3], float("nan"))


def test_report_and_match_coalesced(service):
    valhalla, sm, reqs, levels, matched = service
    reported = sm.ReportMany(reqs, 15)
    before = valhalla.coalesce_stats()
    got = {}
    errors = []

    def work(t):
        try:
            mine = valhalla.SegmentMatcher()
            for i in range(t // 2, 48, 4):
                got[(t % 2, i)] = mine.Report(reqs[i], 15) if t % 2 else mine.Match(reqs[i])
            mine.close()
        except Exception as e:   # noqa: BLE001 (reported below)
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert len(got) == 96
    for i in range(48):
        assert got[(1, i)] == reported[i], i
        assert got[(0, i)] == matched[i], i
    st = valhalla.coalesce_stats()
    assert st["requests"] - before["requests"] == 96 and st["batches"] > before["batches"], (before, st)
