"""The sequential model of the streaming anonymiser (tests/anonymiser_ref.py; DESIGN.md §3 rule 13)
pinned on cases worked out by hand from the Java text (AnonymisingProcessor.java:155-175,
TimeQuantisedTile.java:26-35, Segment.java:50-74).  CPU only; the model is what the GPU tile store
is compared with."""
import pytest

import anonymiser_ref as ar

INV = ar.INVALID_SEGMENT_ID
T = 8                       # every id below is T + (k << 25): one tile (level 0, index 1)
PAIRS = {"A": (T + (1 << 25), 5), "B": (T + (1 << 25), 6), "C": (T + (2 << 25), INV), "D": (T + (3 << 25), 7)}


def _run(letters, privacy):
    m = ar.Anonymiser(3600, privacy, "src", "auto")
    m.add([PAIRS[c] + (100.0 + k, 110.0 + k, 50 + k, 0) for k, c in enumerate(letters.split())])
    files, counts = m.flush()
    if not files:
        return None, counts
    assert list(files) == ["0_3599/0/1"]
    rows = files["0_3599/0/1"].decode().split("\n")
    assert rows[0] == ar.HEADER
    back = {v: k for k, v in PAIRS.items()}
    out = []
    for r in rows[1:]:
        f = r.split(",")
        out.append(back[(int(f[0]), int(f[1]) if f[1] else INV)])
    return " ".join(out), counts


@pytest.mark.parametrize("privacy,given,want", [
    (2, "A A B", "A A B"),
    (2, "A B C", "B C"),
    (2, "A B B", "B B"),
    (2, "B", None),
    (2, "A A B B C", "A A B B C"),
    (3, "A B", None),
    (3, "A A A B", "A A A B"),
    (3, "A B B C", "B B C"),
])
def test_clean_by_hand(privacy, given, want):
    got, counts = _run(given, privacy)
    assert got == want
    assert counts["rows_in"] == len(given.split()) and counts["tiles"] == 1
    assert counts["files"] == (0 if want is None else 1)
    assert counts["rows_kept"] == (0 if want is None else len(want.split()))


def test_clean_keeps_a_lone_row_at_privacy_one():
    assert _run("B", 1)[0] == "B"


def test_truncated_buckets_and_row_text():
    m = ar.Anonymiser(3600, 1, "src", "auto")
    c = m.add([(9, INV, 3599.25, 3600.75, 120, 0)])
    assert c == {"kept": 1, "skipped": 0, "rows": 2, "held": 2}
    files, counts = m.flush()
    assert list(files) == ["0_3599/1/1", "3600_7199/1/1"]
    want = (ar.HEADER + "\n9,,2,1,120,0,3599,3601,src,AUTO").encode()
    assert files["0_3599/1/1"] == want and files["3600_7199/1/1"] == want
    assert counts == {"rows_in": 2, "rows_kept": 2, "tiles": 2, "files": 2,
                      "bytes": len("0_3599/1/1") + len("3600_7199/1/1") + 2 * len(want) + 4}
    assert m.flush() == ({}, {"rows_in": 0, "rows_kept": 0, "tiles": 0, "files": 0, "bytes": 0})


def test_max_is_truncated_not_ceiled():
    m = ar.Anonymiser(3600, 1, "s", "auto")
    m.add([(9, INV, 3700.0, 7199.5, 10, 0)])
    files, _ = m.flush()
    assert list(files) == ["3600_7199/1/1"]
    assert files["3600_7199/1/1"].endswith(b"\n9,,3500,1,10,0,3700,7200,s,AUTO")


def test_numeric_stable_sort():
    m = ar.Anonymiser(3600, 1, "s", "bus")
    same_tile = lambda k: 9 + (k << 25)         # ids 9 and 9 + 2^25 share a tile; next ids 9 and 10 show the numeric order
    m.add([(same_tile(1), 10, 10.0, 20.0, 1, 0), (same_tile(1), 9, 10.0, 21.0, 2, 0), (same_tile(0), 100, 10.0, 22.0, 3, 0),
           (same_tile(1), 9, 10.0, 23.0, 4, 0), (same_tile(1), 10, 10.0, 24.0, 5, 0)])
    files, _ = m.flush()
    rows = files["0_3599/1/1"].decode().split("\n")[1:]
    assert [r.split(",")[:2] + [r.split(",")[4]] for r in rows] == [
        ["9", "100", "3"], ["33554441", "9", "2"], ["33554441", "9", "4"], ["33554441", "10", "1"], ["33554441", "10", "5"]]
    assert all(r.endswith(",s,BUS") for r in rows)


def test_round_and_saturation():
    assert [ar.java_round(x) for x in (0.5, 1.5, 2.5, 0.49999999999999994, 2.4999999999999996)] == [1, 2, 3, 0, 2]
    s = ar.Seg(9, INV, 1.0, 1.0 + 3e9, 1, 0)
    assert ",2147483647,1,1,0,1,3000000001," in ar.row_text(s, "AUTO", "s")


def test_limits_leave_the_store():
    m = ar.Anonymiser(60, 1, "s", "auto")
    m.add([(9, INV, 10.0, 20.0, 1, 0)])
    for bad in [(1 << 63, INV, 10.0, 20.0, 1, 0), (9, 1 << 63, 10.0, 20.0, 1, 0), (9, INV, float("nan"), 20.0, 1, 0),
                (9, INV, 10.0, float("inf"), 1, 0), (9, INV, 10.0, 2.0 ** 53, 1, 0), (9, INV, 10.0, 10.0 + 60 * 65536, 1, 0)]:
        with pytest.raises(ar.LimitError):
            m.add([(9, INV, 30.0, 40.0, 1, 0), bad])
    assert m.held() == 1
    c = m.add([(9, INV, 60.0, 59.0 + 60 * 65536, 1, 0), (9, INV, 5.0, 5.0, 1, 0), (9, INV, 5.0, 6.0, 0, 0)])
    assert c == {"kept": 1, "skipped": 2, "rows": 65536, "held": 65537}
    for kw in (dict(quantisation=59), dict(privacy=0), dict(source="a,b"), dict(source="x" * 65), dict(mode="m" * 17)):
        with pytest.raises(ValueError):
            ar.Anonymiser(**kw)
