"""Input sets that take K3's two kernels through every layer shape.

The candidate radius of a point is max(search_radius, accuracy), so on the 60 x 60 world of 20 m
blocks a search radius of 2 m and a per-point accuracy drawn from ACCURACIES give every candidate
count from 0 to 16, layer by layer, inside one trace.  tests/test_viterbi_ref.py asserts on the CPU
what each set reaches; tests/test_gpu_viterbi_shapes.py runs them on the GPU.

A set is dict(tr=trace arrays as world.generate_traces returns them, opts, topt).
"""
import numpy as np

from reporter_amd import engine, world

ACCURACIES = (-1.0, 5.0, 9.0, 14.0, 22.0, 60.0)
ACC_P = (0.1, 0.2, 0.2, 0.2, 0.15, 0.15)
TURN_FACTOR = 200.0
SEARCH_RADIUS = 2.0

# `many`: 4,101 traces, the hot ones (20-90 points, mixed accuracies) among fillers of 1-3 points.
# Waves of four hot traces of different lengths (400-403, 800-803, 4092-4095), of one hot trace
# among fillers (5, 10, 1001, 2002, 3003), a hot trace in each group position, trace 3 cut to one
# point, and a last wave (4100) with one live group.
MANY_T = 4101
MANY_HOT = (0, 1, 2, 3, 5, 10, 15, 16, 17, 400, 401, 402, 403, 800, 801, 802, 803, 1001, 2002, 3003,
            4092, 4093, 4094, 4095, 4096, 4097, 4099, 4100)
MANY_GROUPS = (400, 800, 4092)          # aligned groups of four hot traces ...
MANY_GROUP_POINTS = (90, 41, 66, 28)    # ... of these lengths

LONG_LENGTHS = (200, 200, 170, 77, 200, 33)
LONG_EMPTY_AT = 150       # trace 1: this point lies 1 degree east, off the map
LONG_SPLICE_AT = 130      # trace 0: from here on the points of trace 4


def dense_world(path):
    """The 60 x 60 world of 20 m blocks (1.2 km square)."""
    return world.build_world(path, 60, 60, 20.0, seed=2, cell_m=20.0)


def cut(tr, lengths):
    """The first lengths[k] points of every trace k."""
    off = tr["trace_off"].astype(np.int64)
    idx = np.concatenate([np.arange(off[k], off[k] + n, dtype=np.int64) for k, n in enumerate(lengths)]
                         + [np.zeros(0, np.int64)])
    out = {name: tr[name][idx] for name in ("lon", "lat", "time", "accuracy", "truth_edge", "truth_off_cm")}
    out["trace_off"] = np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64))]).astype(np.uint32)
    return out


def with_turns(s):
    """The same set with turn costs in every option set."""
    opts = s["opts"].copy()
    opts["turn_penalty_factor"] = TURN_FACTOR
    return dict(tr=s["tr"], opts=opts, topt=s["topt"])


def _options(n, **over):
    return engine.default_options(n, search_radius=SEARCH_RADIUS, **over)


def _draw_accuracy(rng, n):
    return rng.choice(np.array(ACCURACIES, np.float32), size=n, p=ACC_P)


def mixed(path, seed=3):
    """12 traces x 90 points at 0.5 Hz, accuracies drawn per point; four option sets round-robin.
    Trace 3 (interpolation_distance 0, so every point is a state) stands still for four points:
    layers with gc = 0."""
    tr = world.generate_traces(path, n_traces=12, n_points=90, rate_s=2.0, noise_m=4.0, seed=seed)
    rng = np.random.default_rng(seed)
    tr["accuracy"] = _draw_accuracy(rng, 12 * 90)
    o = 3 * 90 + 40
    for name in ("lon", "lat"):
        tr[name][o + 1:o + 4] = tr[name][o]
    opts = _options(4)
    opts[1]["breakage_distance"] = 40.0
    opts[2]["max_route_distance_factor"] = 1.2
    opts[3]["interpolation_distance"] = 0.0
    return dict(tr=tr, opts=opts, topt=(np.arange(12) % 4).astype(np.uint32))


def small_four(path, seed=3):
    """The first four traces of `mixed`, cut to 90, 37, 64 and 5 points: one wave of k_viterbi."""
    s = mixed(path, seed)
    return dict(tr=cut(s["tr"], (90, 37, 64, 5)), opts=s["opts"], topt=s["topt"][:4].copy())


def _metres(lon0, lat0, lon1, lat1):
    """Distance on a sphere, good to a few centimetres at these lengths: it only places the
    breakage distance between the splice's jump and every other step."""
    r = 6378160.0
    p0, p1 = np.radians(lat0), np.radians(lat1)
    a = np.sin((p1 - p0) / 2) ** 2 + np.cos(p0) * np.cos(p1) * np.sin(np.radians(lon1 - lon0) / 2) ** 2
    return 2 * r * np.arcsin(np.sqrt(a))


def long(path, n=6, seed=4):
    """Traces at 1 Hz with accuracy 30 m everywhere (16 candidates on every layer, one layer per
    chunk), chains longer than a backtrace block, ended three ways: by an empty layer (trace 1), by
    gc > breakage with candidates on both sides (trace 0) and by the trace's end.  Trace 2 has one
    chained layer whose gc equals its breakage_distance.  `n` = 4 runs k_viterbi, 6 k_viterbi_w."""
    tr = world.generate_traces(path, n_traces=6, n_points=200, rate_s=1.0, noise_m=4.0, seed=seed)
    tr["accuracy"] = np.full(6 * 200, 30.0, np.float32)
    e = 1 * 200 + LONG_EMPTY_AT
    tr["lon"][e] += 1.0
    tr["accuracy"][e] = 0.5
    a, b = 0 * 200 + LONG_SPLICE_AT, 4 * 200 + LONG_SPLICE_AT
    for name in ("lon", "lat"):
        tr[name][a:200] = tr[name][b:5 * 200]
    step = _metres(tr["lon"][:199], tr["lat"][:199], tr["lon"][1:200], tr["lat"][1:200])
    jump = float(step[LONG_SPLICE_AT - 1])
    rest = float(np.delete(step, LONG_SPLICE_AT - 1).max())
    brk = np.float32(0.5 * (jump + rest))
    assert rest + 5.0 < float(brk) < jump - 5.0, (rest, float(brk), jump)
    opts = _options(3)
    opts[1]["breakage_distance"] = brk
    topt = np.zeros(6, np.uint32)
    topt[0] = 1
    tr = cut(tr, LONG_LENGTHS)
    # trace 2: breakage_distance equal to its largest gc.  gc is rounded to float32 (DESIGN.md §3
    # rule 1) and so is the option, so any gc can be met exactly; "gc > breakage" chains on there,
    # ">=" would break the chain.  gc depends on no option, so the oracle's first pass gives it.
    import meili_oracle as mo
    from reporter_amd import graphfile
    ref = mo.match(graphfile.load(path), mo.Batch(tr["trace_off"], tr["lon"], tr["lat"], tr["time"], tr["accuracy"],
                                                  opts, topt))
    o = int(tr["trace_off"][2])
    top = float(ref["gc"][o + 1:o + int(ref["n_states"][2])].max())
    assert float(np.float32(top)) == top and 10.0 <= top < 100.0, top
    opts[2]["breakage_distance"] = np.float32(top)
    topt[2] = 2
    if n < 6:
        tr = cut(tr, LONG_LENGTHS[:n])
    return dict(tr=tr, opts=opts, topt=topt[:n].copy())


def _many_lengths(rng):
    lengths = rng.integers(1, 4, size=MANY_T)
    lengths[list(MANY_HOT)] = rng.integers(20, 91, size=len(MANY_HOT))
    for g in MANY_GROUPS:
        lengths[g:g + 4] = np.roll(MANY_GROUP_POINTS, MANY_GROUPS.index(g))
    lengths[3] = 1
    return lengths


def many(path, seed=5, empty=False):
    """4,101 traces (k_viterbi; T % 4 == 1), about 8,000 points; two option sets by k % 2.  With
    `empty`, every fifth filler has no points at all."""
    tr = world.generate_traces(path, n_traces=MANY_T, n_points=90, rate_s=2.0, noise_m=4.0, seed=seed)
    rng = np.random.default_rng(seed)
    tr["accuracy"] = _draw_accuracy(rng, MANY_T * 90)
    lengths = _many_lengths(rng)
    if empty:
        filler = np.setdiff1d(np.arange(MANY_T), np.array(MANY_HOT))
        lengths[filler[::5]] = 0
    opts = _options(2)
    opts[1]["max_route_distance_factor"] = 1.2
    return dict(tr=cut(tr, lengths), opts=opts, topt=(np.arange(MANY_T) % 2).astype(np.uint32))


NAMES = ("mixed", "mixed_turns", "small_four", "small_four_turns", "long4", "long6", "many", "many_turns", "empty")
TRACES = dict(mixed=12, mixed_turns=12, small_four=4, small_four_turns=4, long4=4, long6=6, many=MANY_T,
              many_turns=MANY_T, empty=MANY_T)


def build(name, path):
    """The set of that name on the dense world at `path`."""
    base = name[:-6] if name.endswith("_turns") else name
    s = {"mixed": mixed, "small_four": small_four, "long4": lambda p: long(p, 4), "long6": lambda p: long(p, 6),
         "many": many, "empty": lambda p: many(p, empty=True)}[base](path)
    s = with_turns(s) if name.endswith("_turns") else s
    assert len(s["tr"]["trace_off"]) - 1 == TRACES[name]
    return s
