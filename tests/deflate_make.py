"""A small DEFLATE / gzip writer for the inflate tests (DESIGN.md §3 rule 20): members built from
explicit token lists (a literal is an int, a match a (length, distance) pair) as stored, fixed or
dynamic blocks with explicit code lengths, so that the edge cases do not depend on what the
installed zlib chooses to emit.  catalogue() and error_catalogue() are the named streams the host
decoder, the sanitizer program and the GPU tests all read."""
import functools
import random
import struct
import zlib

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


class BitWriter:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, v, n):
        """n bits of v, least significant first (header fields, extra bits)"""
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):
        """a Huffman code: most significant bit first"""
        r = 0
        for _ in range(n):
            r = (r << 1) | (code & 1)
            code >>= 1
        self.bits(r, n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, b):
        assert self.n == 0
        self.out += b

    def done(self):
        self.align()
        return bytes(self.out)


def canonical(lengths):
    """RFC 1951 3.2.2: {symbol: (code, length)} of a list of code lengths"""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def complete_lengths(symbols):
    """a complete code over the symbols: lengths k - 1 and k (one symbol: length 1)"""
    m = len(symbols)
    if m == 1:
        return {symbols[0]: 1}
    k = (m - 1).bit_length()
    short = (1 << k) - m
    return {s: (k - 1 if i < short else k) for i, s in enumerate(symbols)}


def length_symbol(l):
    if l == 258:
        return 285, 0
    s = max(i for i in range(28) if LEN_BASE[i] <= l)
    return 257 + s, l - LEN_BASE[s]


def distance_symbol(d):
    s = max(i for i in range(30) if DIST_BASE[i] <= d)
    return s, d - DIST_BASE[s]


def _emit(w, tokens, lit, dist):
    for t in tokens:
        if isinstance(t, int):
            w.code(*lit[t])
        elif t[0] == "lsym":        # a raw literal/length symbol, nothing after it
            w.code(*lit[t[1]])
        elif t[0] == "dsym":        # a length-3 match with a raw distance symbol
            w.code(*lit[257])
            w.code(*dist[t[1]])
        else:
            s, x = length_symbol(t[0])
            w.code(*lit[s])
            w.bits(x, LEN_EXTRA[s - 257])
            s, x = distance_symbol(t[1])
            w.code(*dist[s])
            w.bits(x, DIST_EXTRA[s])
    w.code(*lit[256])


def stored_block(w, data, final=0, nlen=None):
    assert len(data) <= 65535
    w.bits(final, 1)
    w.bits(0, 2)
    w.align()
    w.raw(struct.pack("<HH", len(data), (len(data) ^ 0xffff) if nlen is None else nlen))
    w.raw(data)


def fixed_block(w, tokens, final=0):
    w.bits(final, 1)
    w.bits(1, 2)
    _emit(w, tokens, canonical(FIXED_LIT), canonical(FIXED_DIST))


def dynamic_header(w, litlens, distlens, final=0, cl_seq=None, hlit=None, hdist=None):
    """litlens (257 .. 286 entries) and distlens (1 .. 30) sent one code-length symbol per length,
    or as cl_seq: a list of (symbol, extra value) written as given"""
    seq = cl_seq if cl_seq is not None else [(l, 0) for l in list(litlens) + list(distlens)]
    used = sorted({s for s, _ in seq})
    if len(used) == 1:              # (an incomplete code-length set is an error)
        used.append(0 if used[0] else 1)
    cl = complete_lengths(used)
    cllens = [cl.get(s, 0) for s in range(19)]
    ncode = max(4, max(i + 1 for i in range(19) if cllens[CL_ORDER[i]]))
    w.bits(final, 1)
    w.bits(2, 2)
    w.bits(len(litlens) - 257 if hlit is None else hlit, 5)
    w.bits(len(distlens) - 1 if hdist is None else hdist, 5)
    w.bits(ncode - 4, 4)
    for i in range(ncode):
        w.bits(cllens[CL_ORDER[i]], 3)
    codes = canonical(cllens)
    for s, x in seq:
        w.code(*codes[s])
        if s >= 16:
            w.bits(x, {16: 2, 17: 3, 18: 7}[s])


def token_symbols(tokens):
    lit, dist = {256}, set()
    for t in tokens:
        if isinstance(t, int):
            lit.add(t)
        elif t[0] == "lsym":
            lit.add(t[1])
        elif t[0] == "dsym":
            lit.add(257)
            dist.add(t[1])
        else:
            lit.add(length_symbol(t[0])[0])
            dist.add(distance_symbol(t[1])[0])
    return sorted(lit), sorted(dist)


def dynamic_block(w, tokens, final=0, litlens=None, distlens=None):
    """litlens / distlens: {symbol: length}; by default a complete code over the symbols the tokens
    use (one symbol: length 1; no distances: one zero length)"""
    ls, ds = token_symbols(tokens)
    litlens = complete_lengths(ls) if litlens is None else litlens
    distlens = (complete_lengths(ds) if ds else {}) if distlens is None else distlens
    ll = [litlens.get(s, 0) for s in range(max(257, max(litlens) + 1))]
    dl = [distlens.get(s, 0) for s in range(max(1, max(distlens) + 1 if distlens else 1))]
    dynamic_header(w, ll, dl, final)
    _emit(w, tokens, canonical(ll), canonical(dl))


def expand(tokens, before=b""):
    """the bytes the tokens stand for, after `before`"""
    out = bytearray(before)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            for _ in range(t[0]):
                out.append(out[-t[1]])
    return bytes(out[len(before):])


def gz_member(deflate, payload, extra=None, name=None, comment=None, hcrc=False, text=False, reserved=0, crc=None, isize=None,
              magic=b"\x1f\x8b", method=8):
    flg = (1 if text else 0) | (2 if hcrc else 0) | (4 if extra is not None else 0) | (8 if name is not None else 0) \
        | (16 if comment is not None else 0) | reserved
    h = magic + bytes([method, flg]) + struct.pack("<IBB", 0x5f000000, 2, 3)
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    if name is not None:
        h += name + b"\0"
    if comment is not None:
        h += comment + b"\0"
    if hcrc:
        h += b"\xde\xad"            # (not the header's CRC: Python's gzip does not check it)
    c = zlib.crc32(payload) if crc is None else crc
    n = len(payload) & 0xffffffff if isize is None else isize
    return h + deflate + struct.pack("<II", c, n)


def gz(payload, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, **header):
    """payload as one member, the DEFLATE stream from zlib"""
    z = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return gz_member(z.compress(payload) + z.flush(), payload, **header)


def trace_lines(n, seed=7):
    """n separated-value trace lines: uuid, time, lat, lon, accuracy"""
    r = random.Random(seed)
    ids = ["veh-%04x%04x" % (r.getrandbits(16), r.getrandbits(16)) for _ in range(max(1, n // 150))]
    out = []
    t = 1483228800
    for _ in range(n):
        t += r.randint(0, 3)
        out.append("%s,%d,%.6f,%.6f,%d" % (r.choice(ids), t, 14.5 + r.random() * 0.2, 121.0 + r.random() * 0.2, r.randint(3, 40)))
    return ("\n".join(out) + "\n").encode()


def text_of(n, seed=1):
    """n bytes of trace text"""
    return trace_lines(n // 30 + 2, seed)[:n]


def _mix():
    r = random.Random(11)
    skew = bytes(min(255, int(r.expovariate(0.08))) for _ in range(120000))
    noise = bytes(r.getrandbits(8) for _ in range(30000))
    return skew + b"\0" * 40000 + noise + trace_lines(1500, 3) + noise + skew[:38000]


def _with_len(payload, total):
    """payload as one member of exactly `total` bytes (the file name pads it)"""
    base = gz(payload, name=b"")
    assert len(base) <= total
    return gz(payload, name=b"n" * (total - len(base)))


@functools.lru_cache(maxsize=None)
def catalogue():
    """[(name, chunk bytes)]: every stream is valid"""
    cat = []
    lines = trace_lines(6000)
    for name, level, strat in (("lines_l0", 0, zlib.Z_DEFAULT_STRATEGY), ("lines_l1", 1, zlib.Z_DEFAULT_STRATEGY),
                               ("lines_l6", 6, zlib.Z_DEFAULT_STRATEGY), ("lines_l9", 9, zlib.Z_DEFAULT_STRATEGY),
                               ("lines_fixed", 6, zlib.Z_FIXED)):
        cat.append((name, gz(lines, level, strat)))
    cat.append(("mix", gz(_mix())))
    r = random.Random(5)
    # distance 32768 and length 258, from an earlier block and across the ring's wrap
    a = bytes(r.getrandbits(8) for _ in range(32768))
    w = BitWriter()
    stored_block(w, a)
    t1 = [(258, 32768), (3, 1), (10, 3), 65, (258, 1)]
    fixed_block(w, t1)
    p = a + expand(t1, a)
    b = bytes(r.getrandbits(8) for _ in range(65536 - 100 - len(p)))
    stored_block(w, b)
    p += b
    t2 = [(258, 32768), (258, 32767), 66, (4, 4)]
    fixed_block(w, t2, final=1)
    p += expand(t2, p)
    cat.append(("far", gz_member(w.done(), p)))
    # 15-bit codes of both kinds
    ls = list(range(97, 109)) + [256, 257, 270, 285]
    litlens = dict(zip([270, 285, 256] + list(range(97, 109)) + [257], list(range(1, 16)) + [15]))
    assert sorted(litlens) == sorted(ls)
    distlens = dict(zip(range(16), list(range(1, 16)) + [15]))
    toks = [97 + (i * 7) % 12 for i in range(400)]
    toks += [(3, DIST_BASE[d]) for d in range(16)] + [(258, 200), (25, 1), 108, (3, 193 + 60)]
    w = BitWriter()
    dynamic_block(w, toks, 1, litlens, distlens)
    cat.append(("deep", gz_member(w.done(), expand(toks))))
    # every block type, three dynamic blocks, an empty stored block, a stored block after unaligned bits
    w = BitWriter()
    t = [[72, 101, 108, 108, 111, (5, 5), 10], [119, 111, (4, 9), 114, 108, 100, 10], [(20, 7), 33, 10], [50, 48, (6, 2), 10]]
    p = b""
    dynamic_block(w, t[0])
    p += expand(t[0], p)
    stored_block(w, b"")
    dynamic_block(w, t[1])
    p += expand(t[1], p)
    fixed_block(w, t[2])
    p += expand(t[2], p)
    stored_block(w, b"stored after bits\n")
    p += b"stored after bits\n"
    dynamic_block(w, t[3], 1)
    p += expand(t[3], p)
    cat.append(("blocks", gz_member(w.done(), p)))
    # the largest stored block
    big = bytes(r.getrandbits(8) for _ in range(65535))
    w = BitWriter()
    stored_block(w, big, 1)
    cat.append(("stored_max", gz_member(w.done(), big)))
    # a one-code distance set; a block of literals with an all-zero distance set
    w = BitWriter()
    t = [[120, 121, 122, (3, 2), (5, 2)], [113, 114, 115]]
    dynamic_block(w, t[0])
    dynamic_block(w, t[1], 1)
    cat.append(("one_dist", gz_member(w.done(), expand(t[0]) + expand(t[1]))))
    # header forms
    one, two, three = text_of(700, 2), text_of(40000, 3), text_of(900, 4)
    cat.append(("three_members", gz(one) + gz(two, 1) + gz(three, 9)))
    cat.append(("empty_member", gz(b"")))
    cat.append(("one_byte", gz(b"\n")))
    cat.append(("padded", gz(one) + b"\0" * 5 + gz(b"") + b"\0" + gz(three) + b"\0" * 512))
    cat.append(("all_flags", gz(one, extra=b"", name=b"trace.csv", comment=b"a comment", hcrc=True, text=True, reserved=0xe0)
                + gz(three, extra=bytes(range(256)) + bytes(44), name=b"", comment=b"", hcrc=True)))
    cat.append(("nothing", b""))
    return cat


@functools.lru_cache(maxsize=None)
def size_catalogue():
    """[(name, chunk bytes)]: outputs at the window's halves and wrap, inputs at the refill size"""
    cat = [("out_%d" % n, gz(text_of(n, n))) for n in (0, 1, 16383, 16384, 16385, 32767, 32768, 32769, 65537)]
    cat += [("in_%d" % n, _with_len(text_of(2500, n), n)) for n in (1023, 1024, 1025)]
    return cat


def _fixed(tokens, final=1):
    w = BitWriter()
    fixed_block(w, tokens, final)
    return w.done()


def _header_only(litlens, distlens, **kw):
    w = BitWriter()
    dynamic_header(w, litlens, distlens, 1, **kw)
    w.bits(0, 32)
    return w.done()


@functools.lru_cache(maxsize=None)
def error_catalogue():
    """[(name, chunk bytes, status)]: one stream per status and cause (0 ok, 1 header, 2 truncated,
    3 malformed block, 4 CRC, 5 size)"""
    good = gz(text_of(3000, 9))
    lit = [0] * 257
    cat = [("bad_magic", b"\x1f\x8c" + good[2:], 1),
           ("one_byte_file", b"\x1f", 1),
           ("bad_method", gz(b"abc", method=7), 1),
           ("cut_header", good[:7], 2),
           ("cut_name", gz(b"abc", name=b"a long file name")[:15], 2),
           ("cut_block", good[:len(good) // 2], 2),
           ("cut_trailer", good[:-3], 2),
           ("cut_stored", gz(text_of(500, 1), 0)[:200], 2)]
    w = BitWriter()
    w.bits(1, 1)
    w.bits(3, 2)
    w.bits(0, 29)
    cat.append(("block_type_3", gz_member(w.done(), b""), 3))
    w = BitWriter()
    stored_block(w, b"hello", 1, nlen=5)
    cat.append(("len_nlen", gz_member(w.done(), b"hello"), 3))
    over = list(lit)
    over[97] = over[98] = over[256] = 1
    cat.append(("over_subscribed", gz_member(_header_only(over, [0]), b""), 3))
    inc = list(lit)
    inc[97] = inc[256] = 2
    cat.append(("incomplete", gz_member(_header_only(inc, [0]), b""), 3))
    no_end = list(lit)
    no_end[97] = no_end[98] = 1
    cat.append(("no_end_of_block", gz_member(_header_only(no_end, [0]), b""), 3))
    ok = list(lit)
    ok[97] = ok[256] = 1
    cat.append(("hlit_287", gz_member(_header_only(ok, [0], hlit=30), b""), 3))
    cat.append(("hdist_31", gz_member(_header_only(ok, [0], hdist=30), b""), 3))
    cat.append(("repeat_first", gz_member(_header_only(ok, [0], cl_seq=[(16, 0)] + [(0, 0)] * 255 + [(1, 0), (0, 0)]), b""), 3))
    cat.append(("repeat_past_end", gz_member(_header_only(ok, [0], cl_seq=[(0, 0)] * 256 + [(1, 0), (18, 127)]), b""), 3))
    w = BitWriter()                 # an empty code-length set: zlib reads one bit per length, then misses symbol 256
    w.bits(1, 1)
    w.bits(2, 2)
    w.bits(0, 14)
    w.bits(0, 12)
    w.bits(0, 258 + 64)
    empty_set = w.done()
    cat.append(("empty_code_length_set", gz_member(empty_set, b""), 3))
    cat.append(("empty_code_length_set_cut", gz_member(empty_set, b"")[:10 + 20], 2))
    cat.append(("symbol_286", gz_member(_fixed([97, ("lsym", 286)]), b"a"), 3))
    cat.append(("distance_symbol_30", gz_member(_fixed([97, 98, 99, ("dsym", 30)]), b"abc"), 3))
    cat.append(("distance_too_far", gz_member(_fixed([97, (3, 2)]), b"aaaa"), 3))
    cat.append(("distance_into_first_member", gz(b"first member\n") + gz_member(_fixed([97, (3, 2)]), b"aaaa"), 3))
    cat.append(("bad_crc", gz(b"some text\n", crc=12345), 4))
    cat.append(("bad_isize", gz(b"some text\n", isize=11), 5))
    cat.append(("bad_crc_second_member", gz(b"one\n") + gz(b"two\n", crc=1), 4))
    cat.append(("garbage_after_trailer", good + b"\0\0garbage", 1))
    return cat
