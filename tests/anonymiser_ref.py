"""The streaming anonymiser restated (DESIGN.md §3 rule 13): the reference's third processor
(AnonymisingProcessor.java:120-153, 155-175, 177-187, 222-266; TimeQuantisedTile.java:26-43;
Segment.java:38-74) as a sequential model in plain Python, one segment at a time.  The GPU tile
store (tilestore.hip) must give this model's files byte for byte, however the segments are cut
into calls.  No JDK is at hand to run the Java, so this model is the specification; the cases of
tests/test_anonymiser_ref.py pin it on results worked out by hand from the Java text.
"""
import math

INVALID_SEGMENT_ID = 0x3FFFFFFFFFFF          # Segment.java:16
HEADER = ("segment_id,next_segment_id,duration,count,length,queue_length,minimum_timestamp,maximum_timestamp,"
          "source,vehicle_type")            # Segment.java:55-57
MAX_SPAN = 65536
I63 = (1 << 63) - 1
INT_MAX, INT_MIN = (1 << 31) - 1, -(1 << 31)


class Seg:
    __slots__ = ("id", "next_id", "min", "max", "length", "queue", "arrival")

    def __init__(self, id, next_id, t0, t1, length, queue, arrival=0):
        self.id, self.next_id, self.min, self.max = int(id), int(next_id), float(t0), float(t1)
        self.length, self.queue, self.arrival = int(length), int(queue), arrival

    def valid(self):                         # Segment.java:38-40
        return self.min > 0 and self.max > 0 and self.max > self.min and self.length > 0 and self.queue >= 0

    def pair(self):                          # what Segment.compareTo orders by (:50-53)
        return (self.id, self.next_id)


def java_round(x):
    """Math.round(double) for finite x: floor(x + 1/2) evaluated exactly (ties up)."""
    fl = math.floor(x)
    return int(fl) + (1 if x - fl >= 0.5 else 0)


def int_value(x):
    """Double.intValue of an integral double: saturating."""
    return max(INT_MIN, min(INT_MAX, int(x)))


def tiles_of(seg, quantisation):
    """TimeQuantisedTile.getTiles (:26-35): (time_range_start, tile_id) per touched bucket; the
    times are truncated (Double.longValue), not floor / ceil."""
    lo, hi = int(seg.min), int(seg.max)
    tile_id = seg.id & 0x1FFFFFF             # Segment.java:34-36
    return [(b * quantisation, tile_id) for b in range(lo // quantisation, hi // quantisation + 1)]


def row_text(seg, mode, source):
    """Segment.appendToStringBuffer (:59-74)."""
    nxt = "" if seg.next_id == INVALID_SEGMENT_ID else str(seg.next_id)
    duration = int_value(float(java_round(seg.max - seg.min)))
    return "\n%d,%s,%d,1,%d,%d,%d,%d,%s,%s" % (seg.id, nxt, duration, seg.length, seg.queue, math.floor(seg.min),
                                              math.ceil(seg.max), source, mode)


def clean(segments, privacy):
    """AnonymisingProcessor.clean (:155-175), the index loop as written; edits the list in place."""
    start = 0
    i = 0
    while i < len(segments):
        s, e = segments[start], segments[i]
        if s.id != e.id or s.next_id != e.next_id or i == len(segments) - 1:
            if i == len(segments) - 1:
                i += 1
            if i - start < privacy:
                del segments[start:i]
                i = start
            else:
                start = i
        i += 1


def tile_name(start, tile_id, quantisation):
    """:185-187 with TimeQuantisedTile.getTileLevel / getTileIndex (:37-43)."""
    return "%d_%d/%d/%d" % (start, start + quantisation - 1, tile_id & 0x7, (tile_id >> 3) & 0x3FFFFF)


class LimitError(ValueError):
    pass


class Anonymiser:
    """process() per segment, punctuate() per flush.  The stated limits of rule 13 raise LimitError
    from add() and leave the store as it was (checked over the whole call first, as the device
    does)."""

    def __init__(self, quantisation=3600, privacy=2, source="smpl_rprt", mode="auto"):
        if privacy < 1:
            raise ValueError("Need a privacy parameter of 1 or more")          # :73-74
        if quantisation < 60:
            raise ValueError("Need quantisation parameter of 60 or more")      # :79-80
        if len(source.encode()) > 64 or len(mode.encode()) > 16 or any(c in x for c in ",\n\r" for x in (source, mode)):
            raise ValueError("source / mode outside the stated limits")
        self.q, self.privacy, self.source, self.mode = quantisation, privacy, source, mode.upper()   # :81
        self.tiles = {}          # (start, tile_id) -> rows in arrival order (the slices concatenated, :233-241)
        self.arrivals = 0

    @staticmethod
    def limit(seg, q):
        if seg.id > I63 or seg.next_id > I63:
            return "id"
        if not (math.isfinite(seg.min) and math.isfinite(seg.max)) or seg.max >= 2.0 ** 53:
            return "time"
        if seg.valid() and int(seg.max) // q - int(seg.min) // q + 1 > MAX_SPAN:
            return "span"
        return None

    def add(self, segs):
        """segs: iterable of (id, next_id, t0, t1, length, queue); returns the counts of rm_tilestore_add."""
        segs = [Seg(*s) for s in segs]
        for s in segs:
            why = self.limit(s, self.q)
            if why:
                raise LimitError(why)
        kept = skipped = rows = 0
        for j, s in enumerate(segs):
            s.arrival = self.arrivals + j
            if not s.valid():                # only valid segments are forwarded (BatchingProcessor.java:126)
                skipped += 1
                continue
            kept += 1
            for key in tiles_of(s, self.q):  # process(): :120-153
                self.tiles.setdefault(key, []).append(s)
                rows += 1
        self.arrivals += len(segs)
        return {"kept": kept, "skipped": skipped, "rows": rows, "held": self.held()}

    def held(self):
        return sum(len(v) for v in self.tiles.values())

    def flush(self):
        """punctuate (:222-266): ({name: body bytes} ordered by (start, tile_id), counts)."""
        files = {}
        rows_in = self.held()
        tiles = len(self.tiles)
        kept = 0
        for key in sorted(self.tiles):
            segments = sorted(self.tiles[key], key=Seg.pair)     # Collections.sort: stable (:246)
            clean(segments, self.privacy)
            if not segments:                                     # :253
                continue
            kept += len(segments)
            body = HEADER + "".join(row_text(s, self.mode, self.source) for s in segments)   # :179-182
            files[tile_name(key[0], key[1], self.q)] = body.encode()
        self.tiles = {}
        nbytes = sum(len(k.encode()) + len(v) + 2 for k, v in files.items())
        return files, {"rows_in": rows_in, "rows_kept": kept, "tiles": tiles, "files": len(files), "bytes": nbytes}
