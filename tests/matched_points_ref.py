"""Independent restatement of the matched-points stage (DESIGN.md §3 rule 9).

Plain Python over numpy ``float32`` scalars, built from ``graphfile.load()`` arrays and the dict
``meili_oracle.match()`` returns.  It uses nothing from the engine: the local frame (``det_cos``
for ``mlon``), the K1 projection, ``road_point`` and ``sq_to`` are written out again here, each
fp32 operation on its own line so that nothing can be contracted or reordered.

``matched_points(g, tr, opts, trace_opt, ref)`` returns one ``REC`` record per input point, in
batch point order.  ``project_on_road`` is K1's projection of a point onto one road; projecting a
state point onto its chosen road must give the oracle's ``cand_sq`` bit for bit and its
``cand_s`` (``check_frame``), which pins the frame to the oracle.
"""
import numpy as np

F = np.float32
NONE = 0xFFFFFFFF
K = 16

REC = np.dtype([("lon", "<f4"), ("lat", "<f4"), ("sq", "<f4"), ("edge", "<u4"), ("off_cm", "<u4"), ("way", "<u4"),
                ("type", "<u4"), ("route_cm", "<u4")])
assert REC.itemsize == 32

UNMATCHED, MATCHED, INTERPOLATED = 0, 1, 2

_DEG = 0.017453292519943295
_COS = (1.0 / 2432902008176640000.0, -1.0 / 6402373705728000.0, 1.0 / 20922789888000.0, -1.0 / 87178291200.0,
        1.0 / 479001600.0, -1.0 / 3628800.0, 1.0 / 40320.0, -1.0 / 720.0, 1.0 / 24.0, -0.5, 1.0)
MLAT = F(110567.0)


def det_cos(x):
    """cos(x), |x| <= pi/2: Taylor to x^20, Horner in x^2 (fp64)."""
    z = x * x
    p = _COS[0]
    for c in _COS[1:]:
        p = p * z + c
    return p


def mlon(lat):
    return F(111320.0 * det_cos(float(lat) * _DEG))


def mode_access(mode):
    return 2 if mode == 3 else (4 if mode == 4 else 1)


class Roads:
    """The graph arrays the stage reads, as plain Python lists (fast scalar indexing)."""

    def __init__(self, g):
        v = g["verts"].reshape(-1, 4)
        self.vlon = [F(x) for x in v[:, 0].copy().view(np.float32)]
        self.vlat = [F(x) for x in v[:, 1].copy().view(np.float32)]
        self.cum = [int(x) for x in v[:, 2]]
        self.voff = [int(x) for x in g["road_vert_off"]]
        self.len = [int(x) for x in g["road_len_cm"]]
        self.fwd = [int(x) for x in g["road_fwd"]]
        self.rev = [int(x) for x in g["road_rev"]]
        e = g["edges"].reshape(-1, 4)
        self.e_info = [int(x) for x in e[:, 2]]
        self.e_road = [int(x) >> 1 for x in e[:, 3]]
        self.e_rev = [int(x) & 1 for x in e[:, 3]]
        self.e_way = [int(x) for x in g["edge_way"]]

    def e_ok(self, e, acc):
        return e != NONE and ((self.e_info[e] >> 16) & 7 & acc) != 0


def road_point(R, r, s):
    """(lon, lat) at s cm along road r: the first shape segment with s <= cum[i+1], or the last."""
    a, b = R.voff[r], R.voff[r + 1] - 1
    i = a
    while i + 1 < b and s > R.cum[i + 1]:
        i += 1
    d = R.cum[i + 1] - R.cum[i]
    t = F(0.0)
    if d > 0:
        t = F(s - R.cum[i]) / F(d)
    lon = R.vlon[i] + t * (R.vlon[i + 1] - R.vlon[i])
    lat = R.vlat[i] + t * (R.vlat[i + 1] - R.vlat[i])
    return lon, lat


def sq_to(plon, plat, ml, qlon, qlat):
    dx = (qlon - plon) * ml
    dy = (qlat - plat) * MLAT
    return dx * dx + dy * dy


def project_segment(R, i, plon, plat, ml):
    """K1's projection of the point onto shape segment i (oracle/meili_oracle.c find_candidates):
    (sq, s) with s = rint(along) clamped to the segment."""
    ax = (R.vlon[i] - plon) * ml
    ay = (R.vlat[i] - plat) * MLAT
    bx = (R.vlon[i + 1] - plon) * ml
    by = (R.vlat[i + 1] - plat) * MLAT
    dx = bx - ax
    dy = by - ay
    l2 = dx * dx + dy * dy
    t = F(0.0)
    if l2 > F(0.0):
        t = -(ax * dx + ay * dy) / l2
        if t < F(0.0):
            t = F(0.0)
        if t > F(1.0):
            t = F(1.0)
    cx = ax + t * dx
    cy = ay + t * dy
    sq = cx * cx + cy * cy
    c0, c1 = R.cum[i], R.cum[i + 1]
    along = F(c0) + t * F(c1 - c0)
    s = int(np.rint(along))
    s = min(max(s, c0), c1)
    return sq, s


def project_on_road(R, r, plon, plat):
    """K1's per-road minimum (sq bits, vertex) over the road's shape segments: (sq, s)."""
    ml = mlon(plat)
    best = None
    for i in range(R.voff[r], R.voff[r + 1] - 1):
        sq, s = project_segment(R, i, plon, plat, ml)
        key = (int(np.float32(sq).view(np.uint32)), i)
        if best is None or key < best[0]:
            best = (key, sq, s)
    return best[1], best[2]


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def search(R, pieces, xmin, plon, plat):
    """The minimum (sq bits, x) over the polyline `pieces` = [(edge, c0, c1)] from route
    coordinate xmin on; ties of the whole key go to the earliest piece, then the lowest shape
    segment.  Returns (sq, x, edge, off_cm, lon, lat)."""
    ml = mlon(plat)
    best = None
    x0 = 0
    for (e, c0, c1) in pieces:
        ln = c1 - c0
        if x0 + ln >= xmin:
            clo = max(c0, c0 + (xmin - x0))
            r, rev, L = R.e_road[e], R.e_rev[e], R.len[R.e_road[e]]
            slo, shi = (L - c1, L - clo) if rev else (clo, c1)
            for i in range(R.voff[r], R.voff[r + 1] - 1):
                if R.cum[i + 1] < slo or R.cum[i] > shi:
                    continue
                _, s = project_segment(R, i, plon, plat, ml)
                s = min(max(s, slo), shi)
                qlon, qlat = road_point(R, r, s)
                sq = sq_to(plon, plat, ml, qlon, qlat)
                c = L - s if rev else s
                x = x0 + (c - c0)
                key = (_bits(sq), x)
                if best is None or key < best[0]:
                    best = (key, sq, x, e, c, qlon, qlat)
        x0 += ln
    return best[1:]


def matched_points(g, tr, opts, trace_opt, ref, trace_errors=None, R=None):
    """One REC per input point (rule 9).  ref: meili_oracle.match() of the same batch."""
    R = R or Roads(g)
    toff = [int(x) for x in tr["trace_off"]]
    P = toff[-1]
    out = np.zeros(P, REC)
    out["edge"] = NONE
    lon, lat = tr["lon"].astype(np.float32), tr["lat"].astype(np.float32)
    choice, cstart = ref["choice"], ref["chain_start"]
    for k in range(len(toff) - 1):
        o, n = toff[k], toff[k + 1] - toff[k]
        if trace_errors is not None and trace_errors[k]:
            continue
        S = int(ref["n_states"][k])
        acc = mode_access(int(opts[int(trace_opt[k])]["mode"]))

        def cont(s):   # state s continues a chain: its slot holds the path of the transition into it
            return 1 <= s < S and not cstart[o + s] and choice[o + s] >= 0

        def path(s):
            a = int(ref["path_off"][o + s])
            return [int(e) for e in ref["path_pool"][a:a + int(ref["path_cnt"][o + s])]]

        for s in range(S):
            a = o + s
            q0 = int(ref["state_orig"][a])
            q1 = int(ref["state_orig"][a + 1]) if s + 1 < S else n
            c = int(choice[a])
            if c < 0:
                continue   # the state and its followers stay unmatched
            r, sa = int(ref["cand_road"][a, c]), int(ref["cand_s"][a, c])
            L = R.len[r]
            if cont(s):
                e = path(s)[-1]
            elif cont(s + 1):
                e = path(s + 1)[0]
            else:
                e = R.fwd[r] if R.e_ok(R.fwd[r], acc) else R.rev[r]
            assert R.e_road[e] == r
            off = L - sa if R.e_rev[e] else sa
            plon, plat = F(lon[o + q0]), F(lat[o + q0])
            qlon, qlat = road_point(R, r, sa)
            out[o + q0] = (qlon, qlat, sq_to(plon, plat, mlon(plat), qlon, qlat), e, off, R.e_way[e], MATCHED, 0)
            if q0 + 1 >= q1:
                continue
            if cont(s + 1):
                pe = path(s + 1)
                cb = int(choice[a + 1])
                sb = int(ref["cand_s"][a + 1, cb])
                pieces = []
                for q, pe_q in enumerate(pe):
                    Lq = R.len[R.e_road[pe_q]]
                    rv = R.e_rev[pe_q]
                    b0 = (Lq - sa if rv else sa) if q == 0 else 0
                    b1 = (Lq - sb if rv else sb) if q + 1 == len(pe) else Lq
                    pieces.append((pe_q, b0, b1))
                assert sum(p[2] - p[1] for p in pieces) == int(ref["route_dist"][a + 1])
            else:
                pieces = [(e, off, L)]
            xmin = 0
            for q in range(q0 + 1, q1):
                plon, plat = F(lon[o + q]), F(lat[o + q])
                sq, x, pe_w, c_w, qlon, qlat = search(R, pieces, xmin, plon, plat)
                out[o + q] = (qlon, qlat, sq, pe_w, c_w, R.e_way[pe_w], INTERPOLATED, x)
                xmin = x
    return out


def check_frame(g, tr, ref, R=None):
    """Project every state point with a choice onto its chosen road as K1 does: the sq bits and
    the offset must be the oracle's cand_sq / cand_s.  Returns the number of states checked."""
    R = R or Roads(g)
    toff = tr["trace_off"]
    lon, lat = tr["lon"].astype(np.float32), tr["lat"].astype(np.float32)
    n = 0
    for k in range(len(toff) - 1):
        o = int(toff[k])
        for s in range(int(ref["n_states"][k])):
            a = o + s
            c = int(ref["choice"][a])
            if c < 0:
                continue
            p = o + int(ref["state_orig"][a])
            sq, sc = project_on_road(R, int(ref["cand_road"][a, c]), F(lon[p]), F(lat[p]))
            assert _bits(sq) == _bits(ref["cand_sq"][a, c]), (k, s, float(sq), float(ref["cand_sq"][a, c]))
            assert sc == int(ref["cand_s"][a, c]), (k, s, sc, int(ref["cand_s"][a, c]))
            n += 1
    return n


def truth_distance_m(g, tr, rec, R=None):
    """Distance in metres from each record's position to the generator's true road position
    (road_point of truth_edge / truth_off_cm), fp64; NaN for unmatched records."""
    R = R or Roads(g)
    d = np.full(len(rec), np.nan)
    for p in range(len(rec)):
        if rec["type"][p] == UNMATCHED:
            continue
        e, c = int(tr["truth_edge"][p]), int(tr["truth_off_cm"][p])
        r = R.e_road[e]
        s = R.len[r] - c if R.e_rev[e] else c
        tlon, tlat = road_point(R, r, s)
        dx = (float(rec["lon"][p]) - float(tlon)) * 111320.0 * np.cos(np.radians(float(tlat)))
        dy = (float(rec["lat"][p]) - float(tlat)) * 110567.0
        d[p] = np.hypot(dx, dy)
    return d
