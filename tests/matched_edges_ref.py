"""Independent restatement of the matched-edges stage (DESIGN.md §3 rule 10).

Plain Python over ``graphfile.load()`` arrays and the dict ``meili_oracle.match()`` returns, in the
manner of ``matched_points_ref.py`` (whose ``Roads`` / ``road_point`` it reuses).  Nothing of the
engine is used: the traversal records are built again from the oracle's paths as
``oracle/meili_oracle.c`` builds them (rule 6; Python floats are IEEE doubles, one operation per
expression in the oracle's order), folded into visits by ``add_trav``'s rule, and the shape is
walked vertex by vertex.

``matched_edges(g, tr, ref)`` returns ``(edge_off, records, shape_off, shape, merged)``: the visits
of trace k are ``records[edge_off[k]:edge_off[k+1]]`` (``REC``), its vertices
``shape[shape_off[k]:shape_off[k+1]]`` (float32 (lon, lat) rows), and ``merged[i]`` is the
(first, last) traversal-record index within its trace that visit i was folded from (dropped
zero-length records count as records: the index is the one K4's windows run over).
"""
import numpy as np

from matched_points_ref import Roads, road_point

NONE = 0xFFFFFFFF
INTERNAL, HAS_SEGMENT, CHAIN_FIRST = 1, 2, 4
FLAG_INTERNAL = 1 << 19   # edge info word (rm_common.hpp kFlagInternal, OG_FLAG_INTERNAL)

REC = np.dtype([("edge", "<u4"), ("way", "<u4"), ("b_cm", "<u4"), ("e_cm", "<u4"), ("t_enter", "<f8"), ("t_exit", "<f8"),
                ("begin_point", "<u4"), ("end_point", "<u4"), ("shape_begin", "<u4"), ("shape_end", "<u4"),
                ("seg_dense", "<u4"), ("seg_off_cm", "<u4"), ("flags", "<u4"), ("len_cm", "<u4")])
assert REC.itemsize == 64


def interp_time(ta, tb, x, D):
    if D == 0:
        return ta
    return ta + (tb - ta) * (float(x) / float(D))


def continues(ref, o, S, s):
    """State s of the trace at slot offset o continues a chain: its slot holds a transition's path."""
    return 1 <= s < S and not ref["chain_start"][o + s] and ref["choice"][o + s] >= 0


def trace_visits(g, R, tr, ref, k):
    """The visits of trace k as dicts (the fields of REC but the shape indices), with "chain" (a
    running chain number within the trace) and "recs" (first, last traversal-record index)."""
    o = int(tr["trace_off"][k])
    S = int(ref["n_states"][k])
    elen = g["edges"].reshape(-1, 4)[:, 1]
    out, chain, open_chain, rec = [], -1, False, 0
    for s in range(S):
        l = o + s
        if not continues(ref, o, S, s):
            open_chain = False          # the list restarts at every chain boundary
            continue
        if not open_chain:
            chain += 1
            open_chain = True
            first_of_chain = True
        la = l - 1
        sa = int(ref["cand_s"][la, ref["choice"][la]])
        sb = int(ref["cand_s"][l, ref["choice"][l]])
        oa, ob = int(ref["state_orig"][la]), int(ref["state_orig"][l])
        ta, tb = float(tr["time"][o + oa]), float(tr["time"][o + ob])
        D = int(ref["route_dist"][l])
        a, ns = int(ref["path_off"][l]), int(ref["path_cnt"][l])
        x = 0
        for q in range(ns):
            e = int(ref["path_pool"][a + q])
            L = int(elen[e])
            rev = R.e_rev[e]
            b0 = (L - sa if rev else sa) if q == 0 else 0
            b1 = (L - sb if rev else sb) if q + 1 == ns else L
            t0 = interp_time(ta, tb, x, D)
            x += b1 - b0
            t1 = interp_time(ta, tb, x, D)
            se = ob if q + 1 == ns else oa
            r = rec
            rec += 1
            if b1 == b0:
                continue                # zero-length pieces carry no information
            if not first_of_chain and out[-1]["edge"] == e and out[-1]["e_cm"] == b0:
                p = out[-1]
                p["e_cm"], p["t_exit"], p["end_point"] = b1, t1, se
                p["recs"] = (p["recs"][0], r)
                continue
            sd = int(g["edge_seg"][e])
            flags = (INTERNAL if R.e_info[e] & FLAG_INTERNAL else 0) | (HAS_SEGMENT if sd != NONE else 0) | (
                CHAIN_FIRST if first_of_chain else 0)
            out.append(dict(edge=e, way=R.e_way[e], b_cm=b0, e_cm=b1, t_enter=t0, t_exit=t1, begin_point=oa, end_point=se,
                            seg_dense=sd, seg_off_cm=int(g["edge_seg_off"][e]), flags=flags, len_cm=L, chain=chain,
                            recs=(r, r)))
            first_of_chain = False
        assert x == D, (k, s, x, D)
    return out


def visit_shape(R, v, shape):
    """Append visit v's vertices to the list `shape` (rule 10) and set its shape indices."""
    e = v["edge"]
    r, rev, L = R.e_road[e], R.e_rev[e], v["len_cm"]
    s_b = L - v["b_cm"] if rev else v["b_cm"]
    s_e = L - v["e_cm"] if rev else v["e_cm"]
    if v["flags"] & CHAIN_FIRST:
        v["shape_begin"] = len(shape)
        shape.append(road_point(R, r, s_b))
    else:
        v["shape_begin"] = len(shape) - 1            # the previous visit's shape_end
    lo, hi = min(s_b, s_e), max(s_b, s_e)
    inner = [i for i in range(R.voff[r], R.voff[r + 1]) if lo < R.cum[i] < hi]
    for i in (reversed(inner) if rev else inner):
        shape.append((R.vlon[i], R.vlat[i]))         # as stored
    shape.append(road_point(R, r, s_e))
    v["shape_end"] = len(shape) - 1


def matched_edges(g, tr, ref, trace_errors=None, R=None):
    R = R or Roads(g)
    T = len(tr["trace_off"]) - 1
    edge_off, shape_off = np.zeros(T + 1, np.uint32), np.zeros(T + 1, np.uint32)
    recs, shapes, merged = [], [], []
    for k in range(T):
        if trace_errors is None or not trace_errors[k]:
            shape = []
            for v in trace_visits(g, R, tr, ref, k):
                visit_shape(R, v, shape)
                recs.append(tuple(v[f] for f in REC.names))
                merged.append(v["recs"])
            shapes.extend(shape)
        edge_off[k + 1] = len(recs)
        shape_off[k + 1] = len(shapes)
    records = np.array(recs, REC) if recs else np.zeros(0, REC)
    shape = np.array(shapes, np.float32).reshape(-1, 2)
    return edge_off, records, shape_off, shape, merged
