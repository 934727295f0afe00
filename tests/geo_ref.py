"""Float64 / long-double references for the stages whose GPU-versus-oracle parity cannot see a
rule both sides got wrong: the state filter, the great-circle distance and K1's candidates
(DESIGN.md §2).  Plain numpy: nothing here comes from oracle/ or rm_common.hpp, there is no grid,
no float32 frame and no hand-written series.  The check_* functions take stage outputs as arrays,
so the same function checks the oracle on the CPU (tests/test_geo_ref.py) and BatchMatcher on the
GPU (tests/test_gpu_geography.py).  They raise AssertionError and return the observed maxima.

Tolerances are derived here, not tuned (u32 = 2^-24 and u64 = 2^-53 are the unit roundoffs of
float32 and float64: the largest relative error of one correctly rounded operation):

gc_bound(h) = h u32 + GC_K u64 R^2 / h.
  The engine computes d = R acos(cosb), cosb = sa sb + ca cb cos(dl), in float64 and rounds d to
  float32: the first term.  An absolute error e in cosb moves d by e R / sin(d / R) = e R^2 / d:
  the second term, with e = GC_K u64 because cosb is within 1e-5 of 1 at every distance a trace
  steps.  GC_K counts the roundings that reach cosb at full weight: the three products and the sum
  (4), and the final rounding of each of the four latitude series sa, sb, ca, cb (4); the series'
  inner roundings and cos(dl)'s (dl < 1e-3: the series is 1 - z/2 to 1e-14) enter scaled by the
  terms' shares sa sb and ca cb of cosb, which sum to 1, and are inside the slack of taking every
  rounding at its worst and with one sign.  GC_K = 8: 3.3 mm at 11 m, 0.4 mm at 100 m.  acos's own
  roundings (1 - c is exact above 1/2, then a square root and a series in y^2 < 1e-10) are
  relative, a few u64 of d, and vanish beside h u32.

frame_delta(r, L) = 10 * 4 u32 (r + L).
  K1 projects in float32 in the local frame at the point.  A coordinate there is at most r + L
  metres (L: the longest shape piece): the point is within r of the piece's nearest point, which
  is within L of either end.  Each coordinate of the nearest point carries about 3 roundings (the
  scaling by mlon or mlat, t dx, the sum; the difference of two float32 degrees that close is
  exact), plus mlon's own rounding to float32: 4 u32 (r + L).  The error of t itself moves the
  nearest point along the piece, which changes the distance only in second order (or not at all
  where t was clamped), and sq's three roundings are relative to a distance of at most r.  Ten
  times that worst case: 0.45 mm at r = 50 m and 140 m pieces, 0.8 mm at 200 m.
"""
import numpy as np

R_EARTH = 6378160.187          # Valhalla midgard kRadEarthMeters
M_PER_LON_EQ = 111320.0        # rule 2: metres per degree of longitude at the equator
M_PER_LAT = 110567.0           # rule 2: metres per degree of latitude
MAX_RADIUS = 200.0             # the cap of a point's search radius
K = 16                         # candidates kept per state
NONE = 0xFFFFFFFF
U32 = 2.0 ** -24
U64 = 2.0 ** -53
GC_K = 8


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def haversine(lon_a, lat_a, lon_b, lat_b):
    """Great-circle metres between the float32-rounded points, in long double."""
    ld = np.longdouble
    rad = ld(4) * np.arctan(ld(1)) / ld(180)   # np.pi is a double: pi in long double from the arctangent
    lo_a, la_a, lo_b, la_b = (f32(x).astype(ld) * rad for x in (lon_a, lat_a, lon_b, lat_b))
    sp, sl = np.sin((la_b - la_a) / 2), np.sin((lo_b - lo_a) / 2)
    h = sp * sp + np.cos(la_a) * np.cos(la_b) * sl * sl
    return 2 * ld(R_EARTH) * np.arcsin(np.sqrt(h))


def gc_bound(h):
    """The derived bound on |gc - haversine| at distance h (module docstring); inf at h = 0."""
    h = np.asarray(h, np.float64)
    with np.errstate(divide="ignore"):
        return h * U32 + GC_K * U64 * R_EARTH * R_EARTH / h


def frame_delta(r, longest_piece_m):
    return 10.0 * 4.0 * U32 * (np.asarray(r, np.float64) + longest_piece_m)


def point_radius(search_radius, accuracy):
    """A point's search radius: the larger of the option and a given accuracy, capped at 200 m."""
    acc, sr = np.asarray(accuracy, np.float32), np.asarray(search_radius, np.float32)
    r = np.where(acc > sr, acc, sr).astype(np.float32)
    return np.clip(r, 0.0, MAX_RADIUS).astype(np.float64)


def mode_access(mode):
    return {3: 2, 4: 4}.get(int(mode), 1)


def state_layout(trace_off, n_states, state_orig):
    """(slot, point, trace) of every state, in slot order."""
    off = np.asarray(trace_off, np.int64)
    ns = np.asarray(n_states, np.int64)
    trace = np.repeat(np.arange(len(ns)), ns)
    first = np.cumsum(ns) - ns
    slot = off[trace] + np.arange(int(ns.sum())) - first[trace]
    return slot, off[trace] + np.asarray(state_orig, np.int64)[slot], trace


def check_states(lon, lat, trace_off, n_states, state_orig, interpolation_distance):
    """The state filter: a trace's first point is a state; a point is skipped only if it is nearer
    than interpolation_distance to the last state, and the next state is no nearer than that, both
    within gc_bound.  No exclusions.  Returns the largest skipped and smallest kept distance."""
    off = np.asarray(trace_off, np.int64)
    worst_skip, worst_keep, skipped, kept = 0.0, np.inf, 0, 0
    for k in range(len(off) - 1):
        o, n, ns = int(off[k]), int(off[k + 1] - off[k]), int(n_states[k])
        if n == 0:
            assert ns == 0, k
            continue
        so = np.asarray(state_orig[o:o + ns], np.int64)
        assert ns >= 1 and so[0] == 0 and (np.diff(so) > 0).all() and so[-1] < n, (k, so)
        is_state = np.zeros(n, bool)
        is_state[so] = True
        last = np.maximum.accumulate(np.where(is_state, np.arange(n), 0))   # the state at or before i
        prev = np.where(is_state, np.concatenate([[0], last[:-1]]), last)   # ... before a state: the previous one
        i = np.arange(1, n)
        h = haversine(lon[o + prev[i]], lat[o + prev[i]], lon[o + i], lat[o + i]).astype(np.float64)
        b = gc_bound(h)
        st = is_state[i]
        bad = np.where(st, h < interpolation_distance - b, h >= interpolation_distance + b)
        if bad.any():
            j = int(i[np.nonzero(bad)[0][0]])
            raise AssertionError("trace %d point %d is %s at %.6f m from state point %d (bound %.2e m)" % (
                k, j, "a state" if is_state[j] else "skipped", h[j - 1], prev[j], b[j - 1]))
        if (~st).any():
            worst_skip = max(worst_skip, float(h[~st].max()))
        if st.any():
            worst_keep = min(worst_keep, float(h[st].min()))
        skipped += int((~st).sum())
        kept += int(st.sum()) + 1
    return dict(states=kept, skipped=skipped, max_skipped_m=worst_skip, min_kept_m=worst_keep)


def check_gc(lon, lat, trace_off, n_states, state_orig, gc):
    """gc of every state after a trace's first against the haversine of the two state points."""
    slot, point, trace = state_layout(trace_off, n_states, state_orig)
    later = np.concatenate([[False], trace[1:] == trace[:-1]])
    a, b = point[np.nonzero(later)[0] - 1], point[later]
    h = haversine(lon[a], lat[a], lon[b], lat[b])
    got = np.asarray(gc, np.float64)[slot[later]]
    err = np.abs(got.astype(np.longdouble) - h).astype(np.float64)
    h = h.astype(np.float64)
    bound = gc_bound(h)
    same = h == 0.0
    assert (got[same] == 0.0).all()
    bad = (err > bound) & ~same
    if bad.any():
        j = int(np.nonzero(bad)[0][0])
        raise AssertionError("gc %.9f against haversine %.9f at state slot %d: off by %.3e m, bound %.3e m (%d of %d)" % (
            got[j], h[j], slot[later][j], err[j], bound[j], int(bad.sum()), len(h)))
    ok = ~same
    return dict(transitions=int(ok.sum()), max_err_m=float(err[ok].max()) if ok.any() else 0.0,
                max_err_over_bound=float((err[ok] / bound[ok]).max()) if ok.any() else 0.0,
                min_m=float(h[ok].min()) if ok.any() else 0.0)


class Pieces:
    """Every shape piece of every road a mode can use, from the graph's arrays."""

    def __init__(self, g, access):
        v = g["verts"].reshape(-1, 4)
        E = g["edges"].reshape(-1, 4)

        def usable(e):
            e = np.asarray(e, np.int64)
            ok = e != NONE
            info = E[np.where(ok, e, 0), 2]
            return ok & ((((info >> 16) & 7) & access) != 0)

        self.road_ok = usable(g["road_fwd"]) | usable(g["road_rev"])
        a = np.nonzero(v[:, 3] != NONE)[0]
        a = a[self.road_ok[v[a, 3]]]
        self.a = a
        self.piece_road = v[a, 3].astype(np.int64)
        assert (np.diff(self.piece_road) >= 0).all()                     # a road's pieces are contiguous
        self.start = np.nonzero(np.concatenate([[True], np.diff(self.piece_road) != 0]))[0]
        self.roads = self.piece_road[self.start]                         # the column -> road id
        self.column = np.full(len(g["road_len_cm"]), -1, np.int64)
        self.column[self.roads] = np.arange(len(self.roads))
        lon, lat = v[:, 0].view(np.float32).astype(np.float64), v[:, 1].view(np.float32).astype(np.float64)
        self.alon, self.alat, self.blon, self.blat = lon[a], lat[a], lon[a + 1], lat[a + 1]
        self.acum, self.bcum = v[a, 2].astype(np.float64), v[a + 1, 2].astype(np.float64)
        self.longest_m = float((self.bcum - self.acum).max()) / 100.0


def brute_candidates(g, lon, lat, r, access, pieces=None, slack=None):
    """Distance of the float32-rounded points to every road usable by the mode: every shape piece,
    projected in the rule-2 local frame at the point (mlon = 111320 cos(lat) with libm, mlat =
    110567) in float64, the minimum per road; no grid.  Returns (pieces, d, s_lo, s_hi): d[i, c] the
    metres from point i to road pieces.roads[c], and the smallest and largest float64 offset (cm
    along the road) among the road's pieces within slack[i] of that minimum (one offset where the
    nearest piece is unique; r only sizes the default slack, frame_delta)."""
    P = pieces or Pieces(g, access)
    lon, lat = f32(lon).astype(np.float64), f32(lat).astype(np.float64)
    n = len(lon)
    slack = frame_delta(np.broadcast_to(np.asarray(r, np.float64), (n,)), P.longest_m) if slack is None else slack
    d = np.empty((n, len(P.roads)))
    s_lo, s_hi = np.empty_like(d), np.empty_like(d)
    for c0 in range(0, n, 256):
        sl = slice(c0, min(c0 + 256, n))
        mlon = (M_PER_LON_EQ * np.cos(np.radians(lat[sl])))[:, None]
        ax, ay = (P.alon[None, :] - lon[sl, None]) * mlon, (P.alat[None, :] - lat[sl, None]) * M_PER_LAT
        bx, by = (P.blon[None, :] - lon[sl, None]) * mlon, (P.blat[None, :] - lat[sl, None]) * M_PER_LAT
        dx, dy = bx - ax, by - ay
        l2 = dx * dx + dy * dy
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(l2 > 0.0, -(ax * dx + ay * dy) / l2, 0.0)
        t = np.clip(t, 0.0, 1.0)
        dist = np.hypot(ax + t * dx, ay + t * dy)
        s = P.acum[None, :] + t * (P.bcum - P.acum)[None, :]
        dmin = np.minimum.reduceat(dist, P.start, axis=1)
        close = dist <= np.repeat(dmin, np.diff(np.concatenate([P.start, [len(P.a)]])), axis=1) + slack[sl, None]
        d[sl] = dmin
        s_lo[sl] = np.minimum.reduceat(np.where(close, s, np.inf), P.start, axis=1)
        s_hi[sl] = np.maximum.reduceat(np.where(close, s, -np.inf), P.start, axis=1)
    return P, d, s_lo, s_hi


def check_candidates(g, lon, lat, radius, access, cand_n, cand_road, cand_s, cand_sq):
    """K1's output for n states (arrays of length n, candidates (n, 16)) against brute force.

    With delta = frame_delta(radius, longest piece) per state:
      - every usable road with float64 distance <= r - delta is a candidate; in a state with 16
        candidates, an absent road is instead no nearer than the farthest kept minus delta;
      - every candidate is a usable road, once, with float64 distance <= r + delta;
      - |sqrt(sq) - d64| <= delta, and d64 is non-decreasing along the list within delta;
      - s is within 1 cm + 100 delta of the float64 offset (1 cm: the rounding to whole
        centimetres and the float32 sum A.cum + t (B.cum - A.cum), 0.002 cm at 300 m of road).
        Where two pieces of the road lie within delta of the minimum, the float64 offset is not
        unique and any offset between theirs is taken; `ambiguous_offsets` counts the candidates
        where that range is wider than 1 cm, so the widening is seen to be rare.
    Roads in [r - delta, r + delta] are undecidable and skipped; the caller asserts their share.
    Returns counts and the observed maxima."""
    lon, lat = np.asarray(lon), np.asarray(lat)
    radius = np.broadcast_to(np.asarray(radius, np.float64), lon.shape)
    access = np.broadcast_to(np.asarray(access, np.int64), lon.shape)
    cand_n = np.asarray(cand_n, np.int64)
    out = dict(states=len(lon), pairs=0, skipped=0, candidates=int(cand_n.sum()), full_states=int((cand_n == K).sum()),
               max_dist_err_m=0.0, max_s_err_cm=0.0, max_delta_m=0.0, ambiguous_offsets=0)
    for acc in np.unique(access):
        sel = np.nonzero(access == acc)[0]
        P, d, s_lo, s_hi = brute_candidates(g, lon[sel], lat[sel], radius[sel], int(acc))
        r = radius[sel][:, None]
        delta = frame_delta(radius[sel], P.longest_m)[:, None]
        cn = cand_n[sel]
        n = len(sel)
        kmask = np.arange(K)[None, :] < cn[:, None]
        road = np.asarray(cand_road, np.int64).reshape(-1, K)[sel]
        col = np.where(kmask, P.column[np.where(kmask, road, 0)], 0)
        unusable = kmask & (P.column[np.where(kmask, road, 0)] < 0)
        assert not unusable.any(), "state %d: candidate road %d is not usable with access %d" % (
            sel[np.nonzero(unusable)[0][0]], road[unusable][0], acc)
        rows = np.repeat(np.arange(n), cn)
        cols = col[kmask]
        present = np.zeros(d.shape, bool)
        present[rows, cols] = True
        assert int(present.sum()) == int(cn.sum()), "a road is listed twice in a state"
        near, far = d <= r - delta, d > r + delta
        full = (cn == K)[:, None]
        d_c = np.where(kmask, d[np.arange(n)[:, None], col], np.nan)              # (n, 16) float64 distances
        with np.errstate(all="ignore"):
            d_last = np.where(cn > 0, np.nanmax(np.where(kmask, d_c, -np.inf), axis=1), 0.0)[:, None]

        def first(mask, what):
            if mask.any():
                i, c = (int(x[0]) for x in np.nonzero(mask))
                raise AssertionError("state %d (lon %r lat %r, radius %g, %d candidates): road %d at %.6f m %s (delta %.2e m; %d such)" % (
                    sel[i], float(f32(lon[sel[i]])), float(f32(lat[sel[i]])), radius[sel[i]], cn[i], P.roads[c], d[i, c],
                    what, delta[i, 0], int(mask.sum())))

        first(near & ~present & ~full, "is missing")
        first(~present & full & (d < d_last - delta), "is missing from a full list whose farthest is farther")
        first(present & far, "is a candidate beyond the radius")
        sq = np.where(kmask, np.asarray(cand_sq, np.float64).reshape(-1, K)[sel], 0.0)   # unused slots hold anything
        assert (sq >= 0.0).all()
        derr = np.abs(np.sqrt(sq) - d_c)
        bad = kmask & (derr > delta)
        assert not bad.any(), "sqrt(sq) is off by %.3e m (delta %.2e m) at state %d" % (
            derr[bad].max(), delta[np.nonzero(bad)[0][0], 0], sel[np.nonzero(bad)[0][0]])
        step = d_c[:, 1:] - d_c[:, :-1]
        bad = kmask[:, 1:] & (step < -delta)
        assert not bad.any(), "candidates out of order by %.3e m at state %d" % (-step[bad].min(), sel[np.nonzero(bad)[0][0]])
        s = np.asarray(cand_s, np.float64).reshape(-1, K)[sel]
        lo, hi = s_lo[np.arange(n)[:, None], col], s_hi[np.arange(n)[:, None], col]
        serr = np.where(kmask, np.maximum(np.maximum(lo - s, s - hi), 0.0), 0.0)
        out["ambiguous_offsets"] += int((kmask & (hi - lo > 1.0)).sum())   # two pieces tie within delta, > 1 cm apart
        bad = serr > 1.0 + 100.0 * delta
        assert not bad.any(), "offset off by %.3f cm at state %d (road %d)" % (
            serr[bad].max(), sel[np.nonzero(bad)[0][0]], road[bad][0])
        out["pairs"] += d.size
        out["skipped"] += int((~near & ~far).sum())
        if kmask.any():
            out["max_dist_err_m"] = max(out["max_dist_err_m"], float(derr[kmask].max()))
            out["max_s_err_cm"] = max(out["max_s_err_cm"], float(serr.max()))
        out["max_delta_m"] = max(out["max_delta_m"], float(delta.max()))
    return out


# ---- box probes: points 4 m off the midpoints of shape pieces, radius 5 m ----
PROBE_RADIUS, PROBE_OFFSET, PROBE_PIECES = 5.0, 4.0, 500


def box_probes(g, seed=1, access=1):
    """One-point traces 4 m east, west, north and south of the midpoints of 500 shape pieces (all
    of them where the graph has fewer), without accuracy: K1's padded box (pad = 1.01 r + 0.5 m at
    r = 5 m, against a float32 step of longitude of up to 1.6 m) must still reach the piece.
    Returns (trace set, road of each probe)."""
    P = Pieces(g, access)
    rng = np.random.default_rng(seed)
    pick = np.sort(rng.choice(len(P.a), size=min(PROBE_PIECES, len(P.a)), replace=False))
    mid_lon, mid_lat = 0.5 * (P.alon[pick] + P.blon[pick]), 0.5 * (P.alat[pick] + P.blat[pick])
    mlon = M_PER_LON_EQ * np.cos(np.radians(mid_lat))
    lon = np.concatenate([mid_lon + PROBE_OFFSET / mlon, mid_lon - PROBE_OFFSET / mlon, mid_lon, mid_lon])
    lat = np.concatenate([mid_lat, mid_lat, mid_lat + PROBE_OFFSET / M_PER_LAT, mid_lat - PROBE_OFFSET / M_PER_LAT])
    n = len(lon)
    tr = dict(lon=lon, lat=lat, time=1483228800.0 + np.arange(n, dtype=np.float64), accuracy=np.full(n, -1.0, np.float32),
              trace_off=np.arange(n + 1, dtype=np.uint32))
    return tr, np.tile(P.piece_road[pick], 4)


def check_box_probes(g, tr, probe_road, cand_n, cand_road, access=1):
    """Every probe whose float32-rounded point is within r - delta of its piece's road (float64,
    brute force) has that road among its candidates.  Returns the qualifying share, which the
    caller asserts to be at least 90 %."""
    P, d, _, _ = brute_candidates(g, tr["lon"], tr["lat"], PROBE_RADIUS, access)
    delta = float(frame_delta(PROBE_RADIUS, P.longest_m))
    n = len(probe_road)
    dist = d[np.arange(n), P.column[probe_road]]
    qualifies = dist <= PROBE_RADIUS - delta
    cn = np.asarray(cand_n, np.int64)[:n]
    road = np.asarray(cand_road, np.int64).reshape(-1, K)[:n]
    found = ((road == np.asarray(probe_road, np.int64)[:, None]) & (np.arange(K)[None, :] < cn[:, None])).any(axis=1)
    assert (cn < K).all()
    bad = qualifies & ~found
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise AssertionError("probe %d (lon %r lat %r) is %.4f m from road %d, which is not a candidate (%d probes so)" % (
            i, float(f32(tr["lon"][i])), float(f32(tr["lat"][i])), dist[i], probe_road[i], int(bad.sum())))
    return dict(probes=n, qualify=float(qualifies.mean()), found=int(found.sum()), max_qualifying_m=float(dist[qualifies].max()))
