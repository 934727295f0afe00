"""K3 (Viterbi + breakage) written from DESIGN.md §3 rule 4 in plain Python, on K2's outputs.

It shares nothing with the oracle's C loop or the kernels but the specification:

* a layer without candidates belongs to no chain;
* a layer starts a chain when it is the trace's first, follows a layer without candidates, has
  gc > breakage_distance, or no transition into it is valid;
* otherwise cost_j = min_i fma(d_ij, 1/beta, cost_i) + em_j, the lowest i among equal minima;
  d_ij = |route_m - gc| with route_m = cm * 0.01, or K2's distance term (route_d) with turn costs;
  a source whose cost is +inf (nothing reached it) and an invalid route give no transition;
* em_j = sq_j * 1/(2 sigma_z^2); a chain's winner is its last layer's lowest cost, the lowest j
  among equal costs; the back-pointers give the choice of every layer of the chain.

Every operation is one IEEE double operation (a Python float operation is one), and the fused
multiply-add is float(Fraction(d) * Fraction(1/beta) + Fraction(cost_i)): the sum is exact and
Fraction -> float rounds correctly, so the result is rounded once.

Beside choice and chain_start it returns, per trace, a coverage record: which of the kernels'
paths the trace's layers reach (engine.hip k_viterbi / k_viterbi_w), counted from the reference's
own run.  The tests assert conditions on those counts, so that an input set which stops reaching
a path fails instead of passing quietly.
"""
from fractions import Fraction

import numpy as np

INF = float("inf")
ROUTE_INVALID = 0xFFFFFFFF
MAX_CAND = 16
CHUNK_LAYERS = 16          # layers per staged chunk in both kernels
ROUTES_WAVE = 384          # routes per chunk of k_viterbi_w (kV3Routes)
ROUTES_BATCH = 256         # routes per chunk of k_viterbi (kVitRoutes)
LONG_CHAIN = 65            # a backtrace stages 64 layers per block
K_RANGES = ("<=4", "5-8", "9-16")

# why a layer starts a chain (or holds none), per layer in the coverage record's "cause"
CHAINED, FIRST, EMPTY, BREAKAGE, NO_TRANSITION = 0, 1, 2, 3, 4
CAUSES = ("chained", "first", "empty", "breakage", "no_transition")


def k_range(k):
    return 0 if k <= 4 else (1 if k <= 8 else 2)


def fma(a, b, c):
    """a * b + c rounded once (finite operands)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def chunk_layout(cnt, limit):
    """The greedy chunk layout of v3_layout / vit_layout for one trace: from each chunk's first
    layer, the leading layers whose running sum of routes (cnt[s] = K_A * K_B, 0 for layer 0) fits
    `limit`, at most CHUNK_LAYERS.  Returns (position of every layer in its chunk, length of every
    layer's chunk, chunks cut short by the limit)."""
    S = len(cnt)
    pos, length, cut = [0] * S, [0] * S, 0
    s0 = 0
    while s0 < S:
        total, C = 0, 0
        while C < CHUNK_LAYERS and s0 + C < S and total + cnt[s0 + C] <= limit:
            total += cnt[s0 + C]
            C += 1
        assert C >= 1, "a layer holds at most 256 routes"
        if C < CHUNK_LAYERS and s0 + C < S:
            cut += 1
        for t in range(C):
            pos[s0 + t], length[s0 + t] = t, C
        s0 += C
    return pos, length, cut


def _new_coverage(S):
    return dict(
        cells=np.zeros((3, 3), np.int64),     # chained layers by K_A range x K_B range
        starts=dict(first=0, empty=0, breakage=0, no_transition=0),
        no_transition_ka=np.zeros(3, np.int64),   # no-transition starts by K_A range
        source_ties=0,                        # chained layers where some target's arg-min was tied
        winner_ties=0,                        # chain ends whose lowest cost was tied
        long_chains=dict(empty=0, breakage=0, no_transition=0, end=0),   # >= LONG_CHAIN layers, by what ended them
        k16_layers=0,
        gc_at_breakage=0,                     # chained layers with gc == breakage_distance exactly
        layers=S,
        cause=np.zeros(S, np.uint8))


def _trace(S, kn, sq, toff, gcs, route, route_d, inv2s2, inv_beta, brk, choice, chain_start, cov):
    """One trace: kn / sq / toff / gcs are its layers' candidate counts, emission rows, route
    offsets and gc; choice / chain_start are its slices of the outputs."""
    cost = [None] * S
    bp = [None] * S
    prev_ok = False
    chain_len = 0

    def end_chain(last, why):
        c = cost[last]
        best = min(c)
        w = c.index(best)                      # the lowest j among equal costs
        if c.count(best) > 1:
            cov["winner_ties"] += 1
        if chain_len >= LONG_CHAIN:
            cov["long_chains"][why] += 1
        t = last
        while True:
            choice[t] = w
            if chain_start[t]:
                break
            w = bp[t][w]
            t -= 1

    for s in range(S):
        KB = kn[s]
        cov["k16_layers"] += KB == MAX_CAND
        if KB == 0:
            if prev_ok:
                end_chain(s - 1, "empty")
            chain_start[s] = 1
            cov["starts"]["empty"] += 1
            cov["cause"][s] = EMPTY
            prev_ok, chain_len = False, 0
            continue
        em = [float(sq[s][j]) * inv2s2 for j in range(KB)]
        cause = CHAINED
        if not prev_ok:
            cause = FIRST
        elif gcs[s] > brk:
            cause = BREAKAGE
        else:
            KA = kn[s - 1]
            prev = cost[s - 1]
            base = toff[s]
            nc, nb, tied, any_in = [INF] * KB, [255] * KB, False, False
            for j in range(KB):
                best, arg, ties = INF, -1, 0
                for i in range(KA):
                    ci = prev[i]
                    q = base + i * KB + j
                    if ci == INF:
                        continue
                    if route_d is not None:
                        d = route_d[q]
                        if d == INF:
                            continue
                    else:
                        r = route[q]
                        if r == ROUTE_INVALID:
                            continue
                        d = abs(float(r) * 0.01 - gcs[s])
                    c = fma(d, inv_beta, ci)
                    if c < best:               # the lowest i among equal minima
                        best, arg, ties = c, i, 1
                    elif c == best:
                        ties += 1
                if arg >= 0:
                    nc[j], nb[j], any_in = best + em[j], arg, True
                    tied |= ties > 1
            if any_in:
                cost[s], bp[s] = nc, nb
                cov["cells"][k_range(KA), k_range(KB)] += 1
                cov["source_ties"] += tied
                cov["gc_at_breakage"] += gcs[s] == brk
                chain_len += 1
            else:
                cause = NO_TRANSITION
                cov["no_transition_ka"][k_range(KA)] += 1
        cov["cause"][s] = cause
        if cause != CHAINED:
            if prev_ok:
                end_chain(s - 1, CAUSES[cause])
            chain_start[s] = 1
            cov["starts"][CAUSES[cause]] += 1
            cost[s], bp[s] = em, [255] * KB
            chain_len = 1
        prev_ok = True
    if prev_ok:
        end_chain(S - 1, "end")


def viterbi_ref(trace_off, n_states, cand_n, cand_sq, trans_off, gc, route, route_d, opts, trace_opt=None):
    """K3 of a whole batch.  cand_sq is (P, 16) float32; route_d is None without turn costs.
    Returns (choice int8 [-1 where a layer has no candidates or a slot holds no state],
    chain_start uint8, one coverage record per trace)."""
    trace_off = np.asarray(trace_off, np.int64)
    T = len(trace_off) - 1
    P = int(trace_off[-1])
    choice = np.full(P, -1, np.int8)
    chain_start = np.zeros(P, np.uint8)
    cand_sq = np.asarray(cand_sq).reshape(P, MAX_CAND)
    route_l = np.asarray(route).tolist()
    route_dl = None if route_d is None else np.asarray(route_d, np.float64).tolist()
    covs = []
    for k in range(T):
        o, S = int(trace_off[k]), int(n_states[k])
        op = opts[int(trace_opt[k]) if trace_opt is not None else 0]
        sz, beta = float(op["sigma_z"]), float(op["beta"])
        inv2s2 = 1.0 / (2.0 * sz * sz)
        inv_beta = 1.0 / beta
        brk = float(op["breakage_distance"])
        cov = _new_coverage(S)
        kn = cand_n[o:o + S].astype(np.int64).tolist()
        ch, cs = [-1] * S, [0] * S
        _trace(S, kn, cand_sq[o:o + S].tolist(), trans_off[o:o + S].astype(np.int64).tolist(),
               np.asarray(gc[o:o + S], np.float64).tolist(), route_l, route_dl, inv2s2, inv_beta, brk, ch, cs, cov)
        choice[o:o + S] = ch
        chain_start[o:o + S] = cs
        cnt = [0] + [kn[s - 1] * kn[s] for s in range(1, S)]
        cov["pos_wave"], cov["len_wave"], cov["cut_wave"] = chunk_layout(cnt, ROUTES_WAVE)
        cov["pos_batch"], cov["len_batch"], cov["cut_batch"] = chunk_layout(cnt, ROUTES_BATCH)
        cov["single_wave"] = sum(1 for n in cov["len_wave"] if n == 1)
        cov["single_batch"] = sum(1 for n in cov["len_batch"] if n == 1)
        cov["kn"] = kn
        covs.append(cov)
    return choice, chain_start, covs


def total(covs):
    """The batch's coverage: the traces' counts added up."""
    out = dict(cells=np.zeros((3, 3), np.int64), no_transition_ka=np.zeros(3, np.int64), starts=dict(first=0, empty=0, breakage=0, no_transition=0),
               long_chains=dict(empty=0, breakage=0, no_transition=0, end=0))
    for name in ("source_ties", "winner_ties", "k16_layers", "gc_at_breakage", "layers", "cut_wave", "cut_batch", "single_wave",
                 "single_batch"):
        out[name] = int(sum(c[name] for c in covs))
    for c in covs:
        out["cells"] += c["cells"]
        out["no_transition_ka"] += c["no_transition_ka"]
        for name in ("starts", "long_chains"):
            for key, v in c[name].items():
                out[name][key] += v
    return out


def summary(tot):
    """One printable line of total()."""
    return ("layers %d cells(KA x KB) %s starts %s no_transition by K_A %s source_ties %d winner_ties %d long_chains %s "
            "cut(384/256) %d/%d single-layer chunks(384/256) %d/%d K16 %d gc==breakage %d" % (
                tot["layers"], tot["cells"].tolist(), tot["starts"], tot["no_transition_ka"].tolist(), tot["source_ties"], tot["winner_ties"],
                tot["long_chains"], tot["cut_wave"], tot["cut_batch"], tot["single_wave"], tot["single_batch"],
                tot["k16_layers"], tot["gc_at_breakage"]))


def explain(covs, trace_off, slot):
    """Where a point slot lies, for a failing comparison: trace, layer, K_A, K_B, why the layer
    starts a chain (or that it is chained), and its position in the chunk of either kernel."""
    trace_off = np.asarray(trace_off, np.int64)
    k = int(np.searchsorted(trace_off, slot, side="right")) - 1
    s = int(slot - trace_off[k])
    c = covs[k]
    if s >= c["layers"]:
        return "slot %d: trace %d point %d holds no state" % (slot, k, s)
    return ("slot %d: trace %d (of wave %d, group %d) layer %d of %d, K_A %d K_B %d, %s, chunk position %d/%d "
            "(384 routes) %d/%d (256 routes)" % (
                slot, k, k // 4, k % 4, s, c["layers"], c["kn"][s - 1] if s else 0, c["kn"][s],
                CAUSES[int(c["cause"][s])], c["pos_wave"][s], c["len_wave"][s], c["pos_batch"][s], c["len_batch"][s]))


def assert_equal(got_choice, got_cs, want_choice, want_cs, covs, trace_off, n_states, what):
    """Exact equality on state slots, naming the first differing slot's shape."""
    from parity_util import state_slots
    sm = state_slots(trace_off, n_states)
    for name, a, b in (("chain_start", got_cs, want_cs), ("choice", got_choice, want_choice)):
        bad = np.nonzero(sm & (np.asarray(a) != np.asarray(b)))[0]
        if len(bad):
            raise AssertionError("%s: %s differs at %d state slots; first: %s: got %d, reference %d" % (
                what, name, len(bad), explain(covs, trace_off, int(bad[0])), int(a[bad[0]]), int(b[bad[0]])))


def run(trace_off, st, opts, trace_opt):
    """viterbi_ref on a dict of stage outputs (the oracle's keys; route_d None without turn costs)."""
    return viterbi_ref(trace_off, st["n_states"], st["cand_n"], st["cand_sq"], st["trans_off"], st["gc"], st["route"],
                       st["route_d"], opts, trace_opt)
