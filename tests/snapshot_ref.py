"""The stream snapshot's layout and checksum restated in numpy (DESIGN.md §3 rule 15;
reporter_amd/csrc/snapshot.hpp), for the tests that take blobs apart and forge them: read() gives
a blob's sections, write() lays sections out again with every checksum recomputed."""
import struct

import numpy as np

MAGIC = 0x0150414E534D5253
VERSION = 1
SEED = np.uint64(0x9E3779B97F4A7C15)
USER, DIR_OFF, DIR_BYTES, SESS_REC, SESS_LON, SESS_LAT, SESS_ACC, SESS_TIME, TILE_ROWS, TILE_META = range(1, 11)
ELEM = {USER: 1, DIR_OFF: 8, DIR_BYTES: 1, SESS_REC: 24, SESS_LON: 4, SESS_LAT: 4, SESS_ACC: 4, SESS_TIME: 8, TILE_ROWS: 64,
        TILE_META: 16}
REC_DTYPE = np.dtype([("vehicle", "<u4"), ("cnt", "<u4"), ("max_sep", "<f4"), ("pad", "<u4"), ("last_update", "<i8")])
META_DTYPE = np.dtype([("arrivals", "<u8"), ("quantisation", "<u4"), ("pad", "<u4")])
HEADER, ENTRY = "<QIIQQ", "<IIQQQQ"
assert struct.calcsize(HEADER) == 32 and struct.calcsize(ENTRY) == 40 and REC_DTYPE.itemsize == 24


def checksum(data):
    """Sum over the 8-byte words w_i (zero-padded) of (w_i ^ SEED) * (2 i + 1) mod 2^64."""
    data = bytes(data)
    w = np.frombuffer(data + b"\0" * (-len(data) % 8), "<u8")
    with np.errstate(over="ignore"):
        return int(((w ^ SEED) * (np.arange(len(w), dtype=np.uint64) * np.uint64(2) + np.uint64(1))).sum(dtype=np.uint64))


def align16(x):
    return (x + 15) & ~15


def read(blob):
    """{kind: bytes} in the blob's order, and its table as [(kind, elem, off, bytes, count, sum)]."""
    magic, version, n, total, tsum = struct.unpack_from(HEADER, blob, 0)
    assert magic == MAGIC and version == VERSION and total == len(blob)
    table = [struct.unpack_from(ENTRY, blob, 32 + 40 * k) for k in range(n)]
    return {e[0]: bytes(blob[e[2]:e[2] + e[3]]) for e in table}, table


def write(sections, counts=None, version=VERSION):
    """The blob of {kind: bytes} (in the dict's order); counts overrides a kind's element count."""
    n = len(sections)
    at = align16(32 + 40 * n)
    table, body = [], b""
    for kind, data in sections.items():
        data = bytes(data)
        count = (counts or {}).get(kind, len(data) // ELEM.get(kind, 1))
        table.append((kind, ELEM.get(kind, 1), at, len(data), count, checksum(data)))
        body += data + b"\0" * (-len(data) % 16)
        at += align16(len(data))
    ents = b"".join(struct.pack(ENTRY, *e) for e in table)
    tsum = checksum(struct.pack(HEADER, MAGIC, version, n, at, 0) + ents)
    head = struct.pack(HEADER, MAGIC, version, n, at, tsum) + ents
    return head + b"\0" * (-len(head) % 16) + body


def retable(blob, edit, header=None):
    """The blob with table entry tuples rewritten by edit(list of lists) and the table's checksum recomputed."""
    magic, version, n, total, _ = struct.unpack_from(HEADER, blob, 0)
    table = [list(struct.unpack_from(ENTRY, blob, 32 + 40 * k)) for k in range(n)]
    edit(table)
    if header:
        version = header.get("version", version)
    ents = b"".join(struct.pack(ENTRY, *e) for e in table)
    tsum = checksum(struct.pack(HEADER, magic, version, n, total, 0) + ents)
    return struct.pack(HEADER, magic, version, n, total, tsum) + ents + bytes(blob[32 + 40 * n:])
