"""RFC 1951 / RFC 1952 in plain Python, written from the RFCs and independent of
reporter_amd/csrc/inflate_core.hpp: the reference of the inflate tests (DESIGN.md §3 rule 20).
inflate(chunk) returns (bytes, status, counts): the bytes of a good chunk (None otherwise), the
rule's status of the first error in stream order, and counts of what the run reached, so that a
test can assert that its inputs exercise what it claims."""
import zlib

OK, HEADER, TRUNCATED, BLOCK, CRC, SIZE, TOO_LARGE = range(7)

_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
              6145, 8193, 12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


class _Stop(Exception):
    def __init__(self, status):
        self.status = status


class _In:
    def __init__(self, data, at):
        self.d, self.at, self.buf, self.cnt = data, at, 0, 0

    def fill(self, n):
        while self.cnt < n and self.at < len(self.d):
            self.buf |= self.d[self.at] << self.cnt
            self.at += 1
            self.cnt += 8

    def bits(self, n):
        if self.cnt < n:
            self.fill(n)
            if self.cnt < n:
                raise _Stop(TRUNCATED)
        v = self.buf & ((1 << n) - 1)
        self.buf >>= n
        self.cnt -= n
        return v

    def to_bytes(self):
        self.bits(self.cnt & 7)
        self.at -= self.cnt >> 3
        self.buf = self.cnt = 0


class _Code:
    """a set of code lengths: `space` left of the code space (< 0 over-subscribed, > 0 incomplete)"""

    def __init__(self, lengths):
        self.maxlen = max(lengths) if lengths else 0
        count = [0] * 16
        for l in lengths:
            count[l] += 1
        self.space = 1
        for l in range(1, 16):
            self.space = self.space * 2 - count[l]
            if self.space < 0:
                return
        code, nxt = 0, [0] * 16
        count[0] = 0
        for l in range(1, 16):
            code = (code + count[l - 1]) << 1
            nxt[l] = code
        self.by_code = {}
        for s, l in enumerate(lengths):
            if l:
                self.by_code[(l, nxt[l])] = s
                nxt[l] += 1
        # bit-reversed codes padded to maxlen: one lookup per symbol
        self.table = {}
        if self.maxlen <= 15 and len(self.by_code) > 0:
            full = {}
            for (l, c), s in self.by_code.items():
                r = int(format(c, "0%db" % l)[::-1], 2)
                for hi in range(1 << (self.maxlen - l)):
                    full[r | (hi << l)] = (s, l)
            self.table = full

    def read(self, src):
        """(symbol, code length); zlib's order: a code is taken once all its bits are there"""
        src.fill(self.maxlen)
        if self.maxlen == 0:
            raise _Stop(BLOCK if src.cnt else TRUNCATED)
        e = self.table.get(src.buf & ((1 << self.maxlen) - 1))
        if e and e[1] <= src.cnt:
            src.buf >>= e[1]
            src.cnt -= e[1]
            return e
        code = 0
        for l in range(1, self.maxlen + 1):
            if l > src.cnt:
                raise _Stop(TRUNCATED)
            code = (code << 1) | ((src.buf >> (l - 1)) & 1)
            if (l, code) in self.by_code:
                raise AssertionError("the table missed a code")
        raise _Stop(BLOCK)


def _sets(src):
    hlit, hdist, hclen = src.bits(5) + 257, src.bits(5) + 1, src.bits(4) + 4
    if hlit > 286 or hdist > 30:
        raise _Stop(BLOCK)
    cl = [0] * 19
    for i in range(hclen):
        cl[_ORDER[i]] = src.bits(3)
    code = _Code(cl)
    if code.maxlen == 0:            # zlib accepts the empty set: each length reads one bit and is zero; then no symbol 256
        for _ in range(hlit + hdist):
            src.bits(1)
        raise _Stop(BLOCK)
    if code.space != 0:
        raise _Stop(BLOCK)
    lens = []
    while len(lens) < hlit + hdist:
        s, _ = code.read(src)
        if s < 16:
            lens.append(s)
            continue
        if s == 16:
            rep = 3 + src.bits(2)
            if not lens:
                raise _Stop(BLOCK)
            prev = lens[-1]
        elif s == 17:
            rep, prev = 3 + src.bits(3), 0
        else:
            rep, prev = 11 + src.bits(7), 0
        if len(lens) + rep > hlit + hdist:
            raise _Stop(BLOCK)
        lens += [prev] * rep
    if lens[256] == 0:
        raise _Stop(BLOCK)
    lit, dist = _Code(lens[:hlit]), _Code(lens[hlit:])
    if lit.space < 0 or (lit.space > 0 and lit.maxlen != 1):
        raise _Stop(BLOCK)
    if dist.space < 0 or (dist.space > 0 and dist.maxlen > 1):
        raise _Stop(BLOCK)
    return lit, dist


_FIXED = None


def _member(src, out, k):
    """one DEFLATE stream onto out (a bytearray of this member's bytes)"""
    global _FIXED
    while True:
        last, kind = src.bits(1), src.bits(2)
        block_at = len(out)
        if kind == 0:
            aligned = (src.cnt & 7) == 5
            src.to_bytes()
            if len(src.d) - src.at < 4:
                raise _Stop(TRUNCATED)
            n = src.d[src.at] | (src.d[src.at + 1] << 8)
            m = src.d[src.at + 2] | (src.d[src.at + 3] << 8)
            if n != (m ^ 0xffff):
                raise _Stop(BLOCK)
            src.at += 4
            if len(src.d) - src.at < n:
                raise _Stop(TRUNCATED)
            out += src.d[src.at:src.at + n]
            src.at += n
            k["stored"] += 1
            k["stored_empty"] += n == 0
            k["stored_max"] += n == 65535
            k["stored_unaligned"] += (not aligned) and k["member_blocks"] > 0
        elif kind == 3:
            raise _Stop(BLOCK)
        else:
            if kind == 1:
                if _FIXED is None:
                    _FIXED = (_Code([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _Code([5] * 32))
                lit, dist = _FIXED
                k["fixed"] += 1
            else:
                lit, dist = _sets(src)
                k["dynamic"] += 1
                k["member_dynamic"] += 1
                k["one_code_dist"] += dist.maxlen == 1 and dist.space > 0
                zero_dist = dist.maxlen == 0
            matches = 0
            while True:
                s, l = lit.read(src)
                k["max_lit_bits"] = max(k["max_lit_bits"], l)
                if s < 256:
                    out.append(s)
                    continue
                if s == 256:
                    break
                if s >= 286:
                    raise _Stop(BLOCK)
                n = _LEN_BASE[s - 257] + (src.bits(_LEN_EXTRA[s - 257]) if _LEN_EXTRA[s - 257] else 0)
                d, l = dist.read(src)
                if d >= 30:
                    raise _Stop(BLOCK)
                k["max_dist_bits"] = max(k["max_dist_bits"], l)
                far = _DIST_BASE[d] + (src.bits(_DIST_EXTRA[d]) if _DIST_EXTRA[d] else 0)
                at = len(out)
                if far > at:
                    raise _Stop(BLOCK)
                matches += 1
                k["max_length"] = max(k["max_length"], n)
                k["max_distance"] = max(k["max_distance"], far)
                k["distance_1"] += far == 1
                k["overlapping"] += far < n
                k["earlier_block"] += at - far < block_at
                pos = k["chunk_bytes"] + at
                k["ring_wrap"] += (pos % 32768) + n > 32768 or ((pos - far) % 32768) + n > 32768
                k["wrap_from_earlier_block"] += (pos % 32768) + n > 32768 and at - far < block_at
                if far >= n:
                    out += out[at - far:at - far + n]
                else:
                    for i in range(n):
                        out.append(out[at - far + i])
            if kind == 2 and zero_dist and matches == 0:
                k["zero_dist_literals"] += 1
        k["member_blocks"] += 1
        if last:
            return


def _header(d, at):
    """past the member header at `at`, as Python's gzip reads it"""
    if d[at:at + 2] != b"\x1f\x8b":
        raise _Stop(HEADER)
    if len(d) - at < 10:
        raise _Stop(TRUNCATED)
    if d[at + 2] != 8:
        raise _Stop(HEADER)
    flg = d[at + 3]
    at += 10
    if flg & 4:
        if len(d) - at < 2:
            raise _Stop(TRUNCATED)
        n = d[at] | (d[at + 1] << 8)
        at += 2
        if len(d) - at < n:
            raise _Stop(TRUNCATED)
        at += n
    for f in (8, 16):
        if flg & f:
            end = d.find(b"\0", at)
            if end < 0:
                raise _Stop(TRUNCATED)
            at = end + 1
    if flg & 2:
        if len(d) - at < 2:
            raise _Stop(TRUNCATED)
        at += 2
    return at, flg


def new_counts():
    return dict.fromkeys(("stored", "fixed", "dynamic", "max_member_dynamic", "max_lit_bits", "max_dist_bits", "max_length",
                          "max_distance", "distance_1", "overlapping", "ring_wrap", "earlier_block", "wrap_from_earlier_block",
                          "members", "empty_members", "one_byte_members", "padding", "stored_empty", "stored_max",
                          "stored_unaligned", "one_code_dist", "zero_dist_literals", "flags_seen", "extra_0", "extra_300",
                          "member_dynamic", "member_blocks", "chunk_bytes"), 0)


def inflate(chunk, counts=None):
    d = bytes(chunk)
    k = new_counts() if counts is None else counts
    k["chunk_bytes"] = 0
    out = []
    at = 0
    try:
        while at < len(d):
            at, flg = _header(d, at)
            k["flags_seen"] |= flg
            k["member_dynamic"] = k["member_blocks"] = 0
            src = _In(d, at)
            body = bytearray()
            _member(src, body, k)
            src.to_bytes()
            at = src.at
            if len(d) - at < 8:
                raise _Stop(TRUNCATED)
            crc = int.from_bytes(d[at:at + 4], "little")
            size = int.from_bytes(d[at + 4:at + 8], "little")
            at += 8
            if zlib.crc32(body) != crc:
                raise _Stop(CRC)
            if len(body) & 0xffffffff != size:
                raise _Stop(SIZE)
            out.append(bytes(body))
            k["members"] += 1
            k["empty_members"] += len(body) == 0
            k["one_byte_members"] += len(body) == 1
            k["max_member_dynamic"] = max(k["max_member_dynamic"], k["member_dynamic"])
            k["chunk_bytes"] += len(body)
            while at < len(d) and d[at] == 0:
                at += 1
                k["padding"] += 1
    except _Stop as e:
        return None, e.status, k
    return b"".join(out), OK, k
