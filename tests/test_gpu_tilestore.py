"""The tile store on the GPU (DESIGN.md §3 rule 13; tilestore.hip) against the sequential model of
tests/anonymiser_ref.py: the ordered mapping name -> body of every flush must be the model's byte
for byte, and the counts of every add and flush the model's, however the segments are cut into
calls.  No matcher is involved: the segments are built here from seeds."""
import numpy as np
import pytest

import anonymiser_ref as ar
from reporter_amd import _lib, engine

pytestmark = pytest.mark.gpu

INV = ar.INVALID_SEGMENT_ID
COLS = ("id", "next_id", "t0", "t1", "length", "queue_length")
DT = (np.uint64, np.uint64, np.float64, np.float64, np.int32, np.int32)


@pytest.fixture(scope="module", autouse=True)
def _lib_ready(built_lib):
    return built_lib


def _arrays(segs):
    return [np.array([s[k] for s in segs], dt) for k, dt in enumerate(DT)]


def _add(store, model, segs):
    got = store.add(*_arrays(segs))
    want = model.add(segs)
    assert got == want, (got, want)
    return got


def _flush(store, model):
    files, counts = store.flush()
    mfiles, mcounts = model.flush()
    assert list(files) == list(mfiles)
    for k in files:
        assert files[k] == mfiles[k], k
    assert counts == mcounts, (counts, mcounts)
    return files, counts


def _pair(q=3600, privacy=2, source="smpl_rprt", mode="auto", **kw):
    return (engine.TileStore(0, q, privacy, source, mode, **kw), ar.Anonymiser(q, privacy, source, mode))


def _chunks(segs, n):
    return [segs[i:i + n] for i in range(0, len(segs), n)]


# ---------------------------------------------------------------- culls
TAILS = [[2, 1], [1, 1, 1], [1, 2], [2, 2, 1], [3, 1], [1, 2, 1]]   # the table's rows with more than one range


def _cull_segments(seed=5, pairs_per_tile=112):
    """3 tile ids x 4 hour buckets; per tile id `pairs_per_tile` (id, next_id) pairs, each 1..5
    times in every file, the arrivals shuffled.  The highest pairs of a file take the sizes of one
    of TAILS behind a closed range of 3; file (tile 0, bucket 0) holds one row, file (tile 0,
    bucket 1) the ranges A B of one row each, file (tile 1, bucket 0) the ranges A B, B twice.
    (112 pairs per tile id: 40 pairs of at most 5 rows in 12 files could not reach 3,000 segments.)"""
    rng = np.random.default_rng(seed)
    segs, layout = [], {}
    for ti, tile in enumerate((8, 8 + (5 << 3), 1 + (77 << 3))):
        ids = [tile + ((1 + k) << 25) for k in range(pairs_per_tile // 4)]
        pairs = sorted((i, n) for i in ids for n in (INV, 9, 10, tile + (3 << 25)))
        for b in range(4):
            if (ti, b) == (0, 0):
                sizes = {pairs[7]: 1}
            elif (ti, b) == (0, 1):
                sizes = {pairs[3]: 1, pairs[4]: 1}
            elif (ti, b) == (1, 0):
                sizes = {pairs[3]: 1, pairs[9]: 2}
            else:
                tail = TAILS[(ti * 4 + b) % len(TAILS)]
                body = pairs[:len(pairs) - len(tail) - 1]
                sizes = {p: int(rng.integers(1, 6)) for p in body}
                sizes[pairs[len(body)]] = 3
                for p, s in zip(pairs[len(body) + 1:], tail):
                    sizes[p] = s
            layout[(ti, b)] = sizes
            for p, s in sizes.items():
                for _ in range(s):
                    t0 = b * 3600 + 10 + float(rng.integers(0, 12000)) / 4.0
                    segs.append((p[0], p[1], t0, t0 + float(rng.integers(1, 2000)) / 4.0, int(rng.integers(1, 3000)),
                                 int(rng.integers(0, 50))))
    order = rng.permutation(len(segs))
    return [segs[i] for i in order], layout


@pytest.fixture(scope="module")
def cull_segs():
    return _cull_segments()


@pytest.mark.parametrize("privacy", [1, 2, 3])
def test_culls(cull_segs, privacy):
    segs, layout = cull_segs
    assert 2500 <= len(segs) <= 3500 and len(layout) == 12
    store, model = _pair(privacy=privacy)
    _add(store, model, segs)
    ms = store.ms()
    assert ms["upload"] > 0 and ms["expand"] > 0 and ms["sort"] == 0, ms
    files, counts = _flush(store, model)
    ms = store.ms()
    assert min(ms[k] for k in ("sort", "cull", "text", "download")) > 0 and ms["upload"] == 0, ms
    assert counts["tiles"] == 12 and counts["rows_in"] == len(segs)
    rows = {k: v.count(b"\n") for k, v in files.items()}
    if privacy == 1:
        assert counts["rows_kept"] == len(segs) and rows["0_3599/0/1"] == 1
    if privacy == 2:
        assert "0_3599/0/1" not in files and rows["3600_7199/0/1"] == 2 and 0 < counts["rows_kept"] < len(segs)
    if privacy == 3:
        assert "3600_7199/0/1" not in files and "0_3599/0/1" not in files and "0_3599/0/6" not in files
        assert counts["files"] == 9
    store.close()


@pytest.mark.parametrize("privacy,given,want", [
    (2, "A A B", 3), (2, "A B C", 2), (2, "A B B", 2), (2, "B", 0), (2, "A A B B C", 5), (3, "A B", 0), (3, "A A A B", 4),
    (3, "A B B C", 3)])
def test_table_rows_as_whole_tiles(privacy, given, want):
    pairs = {"A": (8 + (1 << 25), 5), "B": (8 + (1 << 25), 6), "C": (8 + (2 << 25), INV)}
    store, model = _pair(privacy=privacy, source="src")
    _add(store, model, [pairs[c] + (100.0 + k, 110.5 + k, 50 + k, k) for k, c in enumerate(given.split())])
    files, counts = _flush(store, model)
    assert counts["rows_kept"] == want and counts["files"] == (1 if want else 0)
    store.close()


# ---------------------------------------------------------------- text
def _text_segments():
    segs = []
    for k in range(1, 15):                      # ids of 1 to 14 digits, next_id valid and absent
        for v in (10 ** k - 1, 10 ** (k - 1)):
            if v <= INV:
                segs.append((v, INV if k & 1 else 10 ** (14 - k), 1000.0 + k, 1010.0 + 2 * k, 10 ** (k % 10), k))
    segs.append((INV, 7, 1100.0, 1101.0, 2147483647, 2147483647))
    segs.append((INV, INV, 1100.0, 1107.0, 1, 0))
    for k in range(10):                         # lengths of 1 to 10 digits
        segs.append((123456 + (k << 25), INV - 1, 2000.0, 2031.0, min(10 ** k, 2147483647), 10 ** k // 3))
    for d in (0.5, 1.5, 2.5, 7.5):              # durations at x.5 exactly and just below
        segs.append((40, 41, 3000.0, 3000.0 + d, 5, 0))
        segs.append((40, 41, 3000.0, float(np.nextafter(3000.0 + d, 0.0)), 5, 0))
        segs.append((40, 41, 0.25, float(np.nextafter(0.25 + d, 0.0)), 5, 0))
    segs.append((40, 42, 7000.0, 7200.0, 9, 1))     # max on a bucket edge: also in the next bucket
    segs.append((40, 42, 7000.0, 7199.5, 9, 1))     # half a second before: it is not, though it prints 7200
    segs.append((40, 42, 3599.25, 3600.75, 120, 0))
    segs.append((40, 43, 3500.0, 7300.5, 77, 3))    # three buckets
    segs.append((40, 43, 1.0, 1.0 + 3e9, 77, 3))    # a duration that saturates; 833,334 buckets at q = 3600
    return segs


@pytest.mark.parametrize("source,mode", [("s", "auto"), ("S" * 64, "MotorScooter_16b")])
def test_text(source, mode):
    segs = _text_segments()
    store, model = _pair(q=3600, privacy=1, source=source, mode=mode)
    wide = segs.pop()
    _add(store, model, segs)
    with pytest.raises(RuntimeError, match="65536 time buckets"):
        store.add(*_arrays([wide]))
    files, _ = _flush(store, model)
    assert files["3600_7199/0/5"].count(b"\n40,42,") == 3 and files["7200_10799/0/5"].count(b"\n40,42,") == 1
    assert b"\n40,43,3801,1,77,3,3500,7301," in files["0_3599/0/5"]
    assert b"\n70368744177663,,7,1,1,0,1100,1107," + source.encode() + b"," + mode.upper().encode() in files["0_3599/7/4194303"]
    # the saturating duration, at a quantisation that keeps it inside the span limit
    store2, model2 = _pair(q=86400, privacy=1, source=source, mode=mode)
    _add(store2, model2, [wide])
    f2, c2 = _flush(store2, model2)
    assert c2["rows_kept"] == 34723 and b",2147483647,1,77,3,1,3000000001," in f2["0_86399/0/5"]
    store.close()
    store2.close()


# ---------------------------------------------------------------- shape edges
def _simple(n, tiles, seed, buckets=2):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        tile = int(tiles[int(rng.integers(0, len(tiles)))])
        t0 = float(rng.integers(0, buckets)) * 3600 + 5 + float(rng.integers(0, 3000))
        out.append((tile + (int(rng.integers(1, 4)) << 25), (INV, 3, 12345678901234)[int(rng.integers(0, 3))], t0,
                    t0 + float(rng.integers(1, 900)) / 2.0, int(rng.integers(1, 99999)), int(rng.integers(0, 9))))
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257])
def test_row_totals(n):
    store, model = _pair(privacy=1)
    _add(store, model, _simple(n, [8, 16, 9], n))
    _, counts = _flush(store, model)
    assert counts["rows_in"] == n == counts["rows_kept"]
    store.close()


def test_every_row_opens_a_file_and_one_file_holds_all():
    store, model = _pair(privacy=1, source="x" * 64, mode="m" * 16)
    # 200 rows, each its own file: more than one full wave of file-opening rows, the longest name
    # fields (tile index of 7 digits) and the longest source and mode
    own = [((0x1FFFFFF - k) + (3 << 25), 4611686018427387904 + k, 9007199254000000.0, 9007199254000000.0 + 2, 2147483647,
            2147483647) for k in range(200)]
    _add(store, model, own)
    files, counts = _flush(store, model)
    assert counts["files"] == 200 == counts["tiles"] and max(len(k) for k in files) >= 40
    one = [(8 + (k % 5 << 25), INV, 100.0 + k, 200.0 + k, 1 + k, 0) for k in range(300)]
    _add(store, model, one)
    files, counts = _flush(store, model)
    assert counts["files"] == 1 and counts["rows_kept"] == 300
    store.close()


def test_empty_flush_and_flush_add_flush():
    store, model = _pair(privacy=1)
    files, counts = store.flush()
    assert files == {} and counts == dict.fromkeys(engine.TILE_FLUSH_COUNTS, 0)
    assert store.add(*_arrays([])) == dict.fromkeys(engine.TILE_ADD_COUNTS, 0)
    first, second = _simple(100, [8, 16], 1), _simple(37, [8, 24], 2)
    _add(store, model, first)
    _flush(store, model)
    _add(store, model, second)
    files, counts = _flush(store, model)
    assert counts["rows_in"] == 37
    fresh = ar.Anonymiser(3600, 1)
    fresh.add(second)
    assert files == fresh.flush()[0]
    assert store.flush()[0] == {}
    store.close()


# ---------------------------------------------------------------- cuts and growth
@pytest.mark.parametrize("initial_rows", [1 << 16, 64])
def test_cuts_and_growth(cull_segs, initial_rows):
    segs = cull_segs[0][:700]
    blobs = []
    for cut in (1, 7, 64, 65, len(segs)):
        store, model = _pair(privacy=2, initial_rows=initial_rows)
        held = 0
        for part in _chunks(segs, cut):
            held = _add(store, model, part)["held"]
        assert held == len(segs) and (initial_rows > 64 or held > initial_rows)
        files, _ = _flush(store, model)
        blobs.append(files)
        store.close()
    assert all(list(b.items()) == list(blobs[0].items()) for b in blobs)
    assert len(blobs[0]) >= 8


# ---------------------------------------------------------------- rejections
def test_invalid_segments_are_counted_and_absent():
    store, model = _pair(privacy=1)
    good = _simple(20, [8], 3)
    bad = [(8, INV, 0.0, 5.0, 1, 0), (8, INV, -1.0, 5.0, 1, 0), (8, INV, 5.0, 5.0, 1, 0), (8, INV, 6.0, 5.0, 1, 0),
           (8, INV, 5.0, 6.0, 0, 0), (8, INV, 5.0, 6.0, -3, 0), (8, INV, 5.0, 6.0, 1, -1), (8, INV, 5.0, 0.0, 1, 0)]
    mixed = [x for k in range(8) for x in (good[2 * k], bad[k], good[2 * k + 1])] + good[16:]
    c = _add(store, model, mixed)
    assert c["kept"] == 20 and c["skipped"] == 8
    files, counts = _flush(store, model)
    assert counts["rows_kept"] == c["rows"] and b"\n8,," not in b"".join(files.values())
    store.close()


@pytest.mark.parametrize("bad,message", [
    ((1 << 63, INV, 10.0, 20.0, 1, 0), "above 2\\^63 - 1"),
    ((9, 1 << 63, 10.0, 20.0, 1, 0), "above 2\\^63 - 1"),
    ((9, INV, float("nan"), 20.0, 1, 0), "not finite or max >= 2\\^53"),
    ((9, INV, 10.0, float("inf"), 1, 0), "not finite or max >= 2\\^53"),
    ((9, INV, 10.0, 2.0 ** 53, 1, 0), "not finite or max >= 2\\^53"),
    ((9, INV, 10.0, 10.0 + 3600.0 * 65536, 1, 0), "more than 65536 time buckets"),
])
def test_stated_limits_fail_add_and_leave_the_store(bad, message):
    store, model = _pair(privacy=1)
    before = _simple(50, [8, 9], 4)
    _add(store, model, before)
    with pytest.raises(_lib.RmError, match=message):
        store.add(*_arrays(_simple(10, [8], 5) + [bad] + _simple(10, [9], 6)))
    with pytest.raises(ar.LimitError):
        model.add(_simple(10, [8], 5) + [bad] + _simple(10, [9], 6))
    after = _simple(5, [8], 7)
    assert _add(store, model, after)["held"] == 55
    _flush(store, model)
    store.close()


def test_widest_segment_allowed():
    store, model = _pair(q=60, privacy=1)
    c = _add(store, model, [(9, INV, 60.0, 59.0 + 60 * 65536, 1, 0)])
    assert c["rows"] == 65536
    _, counts = _flush(store, model)
    assert counts["files"] == 65536
    store.close()


@pytest.mark.parametrize("kw,message", [
    (dict(quantisation=59), "quantisation parameter of 60 or more"),
    (dict(privacy=0), "privacy parameter of 1 or more"),
    (dict(source="a,b"), "may not contain"),
    (dict(mode="a\nb"), "may not contain"),
    (dict(source="x" * 65), "longer than 64"),
    (dict(mode="m" * 17), "longer than 16"),
])
def test_creation_limits(kw, message):
    with pytest.raises(_lib.RmError, match=message):
        engine.TileStore(0, **kw)
    with pytest.raises(ValueError):
        ar.Anonymiser(**kw)
