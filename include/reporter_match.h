/* reporter_match.h — C-ABI of libreporter_match.so, the MI355X (gfx950) map
 * matcher that replaces Valhalla/meili behind Open Traffic Reporter.
 *
 * Drop-in boundary (what the reference binds):
 *   valhalla.Configure(conf)             reference py/reporter_service.py:284, py/simple_reporter.py:132
 *       -> rm_configure
 *   valhalla.SegmentMatcher()            reference py/reporter_service.py:52,  py/simple_reporter.py:133
 *       -> rm_matcher_create / rm_matcher_destroy
 *   SegmentMatcher.Match(json) -> json   reference py/reporter_service.py:240, py/simple_reporter.py:166
 *       -> rm_match (+ rm_free for the returned string)
 * The Python package `valhalla/` in this repository binds exactly these through
 * ctypes, so reporter_service.py runs unchanged.
 *
 * Conventions: plain pointers and sizes, no C++ or torch types.  Return 0 on
 * success, non-zero on error; the message is in rm_last_error() (thread-local).
 * Distinct matchers/runners may be used concurrently from different threads;
 * one handle must not be used by two threads at once (the reference keeps one
 * SegmentMatcher per thread, py/reporter_service.py:28-29,51-52).
 */
#ifndef REPORTER_MATCH_H
#define REPORTER_MATCH_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RM_ABI_VERSION 1

/* ---------------- errors / device ---------------- */
const char* rm_last_error(void);
int rm_abi_version(void);
int rm_set_device(int device);  /* device used by the next rm_configure / rm_engine_create */
int rm_device_count(int* count);

/* ---------------- drop-in boundary (valhalla module) ---------------- */
typedef struct rm_matcher rm_matcher;
/* Reads a Valhalla-style JSON config: "meili" defaults (+ per-mode sections) and
 * the graph file ("reporter_amd": {"graph": path} or "mjolnir": {"tile_extract": *.rmg}),
 * loads the graph into HBM.  err/errlen may be NULL. */
int rm_configure(const char* conf_json_path, char* err, size_t errlen);
rm_matcher* rm_matcher_create(void);            /* NULL on error (no configure yet) */
void rm_matcher_destroy(rm_matcher* m);
/* trace_json: {"uuid", "trace":[{"lat","lon","time"[,"accuracy"]}...], "match_options":{...}}
 * *out_json: {"segments":[...]} allocated by the library; release with rm_free. */
int rm_match(rm_matcher* m, const char* trace_json, char** out_json);
/* n traces at once (one GPU launch sequence); outs[i] must each be freed with rm_free. */
int rm_match_batch(rm_matcher* m, const char* const* traces, size_t n, char** outs);
/* rm_match_batch with the n replies in one malloc'd, NUL-terminated buffer: reply i is
 * (*buf)[off[i], off[i+1]) (off: n+1 entries, caller-allocated).  One allocation and one free
 * (rm_free(*buf)) instead of n: the Python binding reads the replies out of one memoryview. */
int rm_match_batch_packed(rm_matcher* m, const char* const* traces, size_t n, char** buf, uint64_t* off);
/* Matched points (DESIGN.md §3 rule 9): where every GPS point of the request ended up on the road,
 * the points the interpolation rule dropped between two states included.  Same request JSON as
 * rm_match; the reply is {"segments":[...],"matched_points":[...]} with the segments of rm_match
 * for that request, byte for byte, and one entry per input point, in input order:
 *   {"lat","lon","type":"matched"|"interpolated","edge_id","way_id","distance_along_edge",
 *    "distance_from_trace_point"}   or   {"lat","lon","type":"unmatched"} (the input position)
 * lat / lon: the snapped position; edge_id: the directed edge; distance_along_edge: the fraction
 * of that edge behind the position (offset / length, as Valhalla's trace_attributes reports it);
 * distance_from_trace_point: metres from the measurement to the snapped position.  Both calls
 * run their requests as one uncoalesced batch (they never enter the coalescer); any failing trace
 * fails the call, naming the trace.  Replies are released with rm_free. */
int rm_match_points(rm_matcher* m, const char* trace_json, char** out_json);
int rm_match_points_batch(rm_matcher* m, const char* const* traces, size_t n, char** outs);
/* Matched edges (DESIGN.md §3 rule 10): the directed edges the match drove, in order, with their
 * times, and the matched polyline -- the "edges" and "shape" of Valhalla's trace_attributes.  Same
 * request JSON as rm_match; the reply is {"segments":[...],"edges":[...],"shape":"..."} with the
 * segments of rm_match for that request, byte for byte.  One entry per edge visit:
 *   {"edge_id","way_id"[,"segment_id"],"begin_shape_index","end_shape_index","begin_trace_index",
 *    "end_trace_index","length"[,"speed"],"start_time","end_time","source_percent_along",
 *    "target_percent_along"[,"internal":true][,"discontinuity":true]}
 * length: kilometres driven on the edge; speed: km/h, present when end_time > start_time;
 * start_time / end_time: distance-interpolated epoch seconds; the two percent_along: the fractions
 * of the edge at which the visit begins and ends; begin / end_shape_index: the visit's first and
 * last vertex in "shape"; begin / end_trace_index: the input point of the matcher state at or
 * before either end; segment_id: the edge's OSMLR segment, when it has one; discontinuity: the
 * visit opens a new chain (the match broke before it).  shape: the encoded polyline of the matched
 * geometry at precision 6 (lat then lon, each llround(v * 1e6)).  Both calls run their requests
 * as one uncoalesced batch; any failing trace fails the call, naming the trace.  Replies are
 * released with rm_free. */
int rm_match_edges(rm_matcher* m, const char* trace_json, char** out_json);
int rm_match_edges_batch(rm_matcher* m, const char* const* traces, size_t n, char** outs);
/* The whole /report reply from one call (DESIGN.md section 3 rule 19; reference
 * py/reporter_service.py:240-243: Match, json.loads, report(), json.dumps): the request rm_match
 * takes in, the complete body out --
 *   {"stats":{...}[,"shape_used":S],"segment_matcher":{"segments":[...],"mode":"auto"},
 *    "datastore":{"mode":"auto","reports":[...]}}
 * (keys and order: rm_report_replies below) -- with report() run on the device in the same run as
 * the match, the trace's end time being its last point's in request order (:81).  threshold_sec is
 * the service's THRESHOLD_SEC: one finite value per call.  match_options.report_levels and
 * match_options.transition_levels (first match_options, first occurrence of either) must be arrays:
 * a number entry that is an integer in -1..7 selects that level, other numbers select nothing, and a
 * missing or non-array value fails the request with the service's own text ("match_options must
 * include report_levels array" / "... transition_levels array"); a non-number entry fails it with
 * "report_levels entries must be numbers" / "transition_levels entries must be numbers" (Python
 * would merely never match it).  A request that fails as an rm_match request fails with that error
 * first.  stats.*.length is the metres as kilometres with three decimals (0 when never assigned) and
 * the times are the shortest decimals that parse back to the same double: round-trip equal to the
 * interpreted reply, not byte equal.
 * rm_report goes through the coalescer as rm_match does; a coalesced batch holds requests of one
 * kind (and one threshold) only, so an rm_match reply is never made by a run with reporting on.
 * rm_report_batch / _packed run their requests as one uncoalesced batch, the device JSON parse
 * included, whatever n is (one request too: unlike rm_match_batch, whose single request takes the
 * coalescer); any failing trace fails the call, naming the trace.  A run above
 * RM_REPLY_DEVICE_MIN_POINTS points (default 65536, the matcher's small-run limit; read per call; 0:
 * always) has its reply text written on the device; a smaller one downloads the records and formats
 * them on the host.  The bytes are the same.  Replies are released with rm_free. */
int rm_report(rm_matcher* m, const char* trace_json, double threshold_sec, char** out_json);
int rm_report_batch(rm_matcher* m, const char* const* traces, size_t n, double threshold_sec, char** outs);
int rm_report_batch_packed(rm_matcher* m, const char* const* traces, size_t n, double threshold_sec, char** buf,
                           uint64_t* off);
/* Diagnostic (the probe and the tests read it; a service needs none of it): the matcher's last
 * rm_report_batch*: [0] reply bytes [1] flagged traces (rm_report_replies)
 * [2] the writer used (1 host, 2 device) [3] the device writer's kernels and scans in microseconds;
 * rm_matcher_timing gives its parse, stage, engine, download, format and total (the device writer's
 * kernels count as format, its downloads as download) */
int rm_report_info(const rm_matcher* m, uint64_t out[4]);
void rm_free(char* p);
/* Host wall times (ms) of the matcher's last uncoalesced rm_match_batch: out[0] JSON parse
 * (single pass, up to 16 host threads), [1] staging into pinned host arrays, [2] engine run
 * (H2D of the batch + every kernel + its size read-backs), [3] segment download (D2H),
 * [4] reply formatting, [5] total. */
int rm_matcher_timing(const rm_matcher* m, double out[6]);
/* Request coalescing (on unless the config sets "reporter_amd": {"coalesce": false}):
 * concurrent rm_match calls from many threads are queued and run as one GPU batch by a
 * dispatcher thread; "coalesce_window_ms" (default 0: take whatever queued while the
 * previous batch ran) and "coalesce_max_traces" (16384) shape the batches.
 * out: [0] batches run [1] requests served [2] largest batch [3] requests queued now. */
int rm_coalesce_stats(uint64_t out[4]);
/* Dispatcher wall time (ms, summed over the batches since rm_configure): [0] staging the parsed
 * points into pinned memory, [1] the engine run (uploads, kernels, size read-backs), [2] the
 * segment download, [3] reply formatting.  Parsing runs on the calling threads, not here. */
int rm_coalesce_timing(double out[4]);

/* ---------------- matcher options (layout of rm::MatchOptions) ---------------- */
typedef struct {
  int32_t mode;  /* 0 auto, 1 bus, 2 motor_scooter, 3 bicycle, 4 pedestrian */
  float sigma_z, beta, search_radius, gps_accuracy, breakage_distance, interpolation_distance,
      max_route_distance_factor, max_route_time_factor, turn_penalty_factor;
} rm_options;
void rm_default_options(rm_options* o);

/* ---------------- synthetic world (host only; no GPU needed) ---------------- */
typedef struct {
  uint32_t rows, cols;
  double block_m;
  uint64_t seed;
  double center_lat, center_lon, jitter;
  uint32_t arterial_every, highway_every;
  double segment_max_m, internal_m, service_frac, oneway_frac, curve_frac, cell_m;
} rm_world_params;
void rm_default_world_params(rm_world_params* p);
int rm_world_build(const rm_world_params* p, const char* out_path);
/* counts of a graph file: nodes, edges, roads, verts, segments, cells, cell items */
int rm_graph_info(const char* graph_path, uint64_t out[7]);
/* OpenStreetMap exchange (graph_osm.cpp; the reference builds its Valhalla tiles from OSM,
 * py/get_tiles.py:30-102, py/simple_reporter.py:36-49).  rm_graph_export_osm writes an .rmg
 * graph as OSM XML: routing tags (highway, maxspeed, oneway, access) on one way per road,
 * exact reporter:* tags, one type=osmlr relation per OSMLR segment, the grid geometry in a
 * type=reporter_grid relation.  rm_graph_import_osm reads OSM XML into an .rmg: an exported
 * file comes back bit-identical; any other OSM XML is split into roads at intersections with
 * speeds / access from its tags and a grid index of cell_m metres (OSMLR segments only where
 * osmlr relations give them). */
int rm_graph_export_osm(const char* graph_path, const char* osm_path);
/* The same OSM elements as OSM PBF (the input valhalla_build_tiles reads, reference
 * Dockerfile:42-49): zlib-deflated blobs, an OSMHeader (OsmSchema-V0.6, DenseNodes), dense
 * nodes at nanodegree granularity (exact float coordinates; a reporter:ll tag where nanodegrees
 * would not bring a float back), ways and relations with packed delta-coded refs. */
int rm_graph_export_pbf(const char* graph_path, const char* pbf_path);
/* OSM XML or PBF (told apart by content) -> .rmg. */
int rm_graph_import_osm(const char* osm_path, const char* graph_path, double cell_m);
/* A seeded irregular city written as generic OSM (osm_city.cpp), with no reporter:* tags, so
 * rm_graph_import_osm ingests it as it would an extract: a jittered junction lattice of curved
 * multi-vertex ways, diagonal avenues crossing at 9-road hubs, roundabouts, boulevards of one-way
 * carriageway pairs, one-way streets, dead ends, service loops, foot / cycle paths, a trunk road
 * on bridges joined at ramps, type=osmlr relations on part of the ways only, OSM ids in shuffled
 * chunks.  pbf != 0 writes PBF, else XML (the same elements). */
typedef struct {
  uint32_t rows, cols;
  double block_m;
  uint64_t seed;
  double center_lat, center_lon, jitter;
  uint32_t primary_every, secondary_every, boulevard_every, diagonal_every;
  double roundabout_frac, drop_frac, oneway_frac, spur_frac, service_frac, footway_frac, osmlr_local_frac,
      way_max_m;
  uint32_t trunk;
} rm_city_params;
void rm_default_city_params(rm_city_params* p);
int rm_osm_city_write(const rm_city_params* p, const char* osm_path, int pbf);

typedef struct {
  uint32_t n_traces, n_points;
  double rate_s, noise_m;
  uint64_t seed;
  int32_t mode;
  int64_t start_epoch;
  uint32_t threads;
} rm_trace_params;
void rm_default_trace_params(rm_trace_params* p);
/* Arrays sized n_traces*n_points; truth_* may be NULL. */
int rm_traces_generate(const char* graph_path, const rm_trace_params* p, double* lon, double* lat, double* time,
                       float* accuracy, uint32_t* truth_edge, uint32_t* truth_off_cm);
/* p->n_traces traces; slot k holds trace ids[k] of the seeded set (identical to what
 * rm_traces_generate puts at index ids[k]): one rank generates just its uuid shard. */
int rm_traces_generate_ids(const char* graph_path, const rm_trace_params* p, const uint32_t* ids, double* lon,
                           double* lat, double* time, float* accuracy, uint32_t* truth_edge, uint32_t* truth_off_cm);

/* ---------------- batched array API (bench / batch pipeline / parity tests) ---------------- */
typedef struct rm_engine rm_engine;
typedef struct rm_runner rm_runner;

rm_engine* rm_engine_create(const char* graph_path, int device);
void rm_engine_destroy(rm_engine* e);
uint32_t rm_engine_n_segments(const rm_engine* e);
int rm_engine_segment_ids(const rm_engine* e, uint64_t* ids); /* n_segments ids (dense index -> OSMLR id) */
/* Route balls (K2's lookup tier): per node and travel mode, exact shortest (dist, time) keys
 * to every node within `radius_m`, built once per mode on first use.  Transitions whose
 * route bound fits the radius are answered by table probes instead of a bounded search;
 * results are identical either way.  radius_m 0 disables the tier.  Set before the first
 * run (modes already built keep their tables).  0..10000 m.  Default: env RM_BALL_RADIUS_M,
 * else rm_graph_auto_ball_radius of the graph. */
int rm_engine_set_ball_radius(rm_engine* e, double radius_m);
/* Host-only: the engine's automatic radius for a graph file — the largest of 2000 m (meili's
 * default breakage distance, so every default-bounded transition is a table probe), 1500,
 * 1000, 700, 500 m whose estimated tables stay within 72 GiB per mode (RM_BALL_BUDGET_GB) and
 * 2^33 rows; else 400 m. */
int rm_graph_auto_ball_radius(const char* graph_path, double* radius_m);
/* Host-only: the radius a travel mode's tables are built at when avail_gb GiB of HBM are left
 * for them — the largest of start_m and the radii below it (2000, 1500, 1000, 700, 500, 400,
 * 300, 200 m) whose sampled tables for that mode (+10 %) fit avail_gb and 2^33 rows; 0 when none
 * does (the mode's transitions then run in the search tiers).  The engine applies it per mode
 * with avail = min(per-mode budget, half the device's HBM less earlier modes' tables, free HBM
 * less 4 GiB); auto and bus share one build. */
int rm_graph_fit_ball_radius(const char* graph_path, int mode, double start_m, double avail_gb, double* radius_m);
/* Host-only: sampled ball statistics of `mode` at radius_m (bounded searches from 256 nodes):
 * out[3] = mean nodes per ball, estimated table bytes of all nodes, fraction of balls above
 * 4096 nodes. */
int rm_graph_ball_sample(const char* graph_path, int mode, double radius_m, double out[3]);
/* out[6]: radius m, keys stored, table entries (16 B each), nodes without a table, build ms,
 * 1 when the tables were built on the GPU (small balls on large graphs; env RM_BALL_BUILD=host|gpu) */
int rm_engine_ball_stats(const rm_engine* e, int mode, double out[6]);
/* K1's spatial index: the graph file's grid with each cell split f x f (*f = 1: the file's grid),
 * chosen at upload to minimise the items a default-radius query reads (RM_GRID_SPLIT overrides).
 * It changes which grid items are read, never which roads are found. */
int rm_engine_grid_split(const rm_engine* e, uint32_t* f);
/* K1's second grid (engine.hip Engine::k1_grid): its split f (0: none) and the batch query
 * radius (m) from which a batch takes it instead of the default one.  New in round 5: no
 * reference call site (the reference has no grid index; Valhalla's meili owns its own). */
int rm_engine_grid_alt(const rm_engine* e, uint32_t* f, float* radius_m);
/* turn rows (DESIGN.md §3 rule 3b) built so far: bit per travel mode, and each mode's build ms */
int rm_engine_turn_rows(const rm_engine* e, uint32_t* mode_mask, double* build_ms /*5*/);
/* Host-only: the grid refinement an engine would choose for a graph file. */
int rm_graph_grid_split(const char* graph_path, uint32_t* f);
/* The engine's own tables of `mode` (built by a run that used the mode), probed on the device as
 * K2 probes them: keys[2i], keys[2i+1] from node from[i] to road[i]'s node0 / node1, all-ones
 * outside the ball or for a node without a table; preds (may be NULL) gets the rows' canonical
 * predecessor indices of node0 / node1 (7: none stored).  Compare with rm_balls_lookup. */
int rm_engine_ball_lookup(rm_engine* e, int mode, uint64_t n, const uint32_t* from, const uint32_t* road,
                          uint64_t* keys, uint8_t* preds);
/* Host-only check of the ball tables (no GPU): builds the balls of `mode` for the graph
 * file and looks up n (from node, road) pairs the way the K2 kernel probes them;
 * keys[2i], keys[2i+1] = dist_cm << 32 | time_ms from `from` to the road's node0 / node1,
 * all-ones for an endpoint outside the ball (or `from` without a table).  preds (may be NULL):
 * preds[2i], preds[2i+1] = the index, among the endpoint's in-edges in edge-id order, of its
 * canonical predecessor in the search from `from` (smallest-id usable in-edge u -> v with
 * key(from -> u) + key(u -> v) == key(from -> v)); 7 when the endpoint is `from`, outside the
 * ball, or the index is 7 or more.  Returns 0 / -1. */
int rm_balls_lookup(const char* graph_path, int mode, double radius_m, uint64_t n, const uint32_t* from,
                    const uint32_t* road, uint64_t* keys, uint8_t* preds);

rm_runner* rm_runner_create(rm_engine* e);
void rm_runner_destroy(rm_runner* r);

typedef struct {
  uint32_t n_traces;
  const uint32_t* trace_off;  /* n_traces+1 */
  const float* lon;           /* degrees */
  const float* lat;
  const double* time;         /* epoch seconds */
  const float* accuracy;      /* metres, < 0 when absent */
  uint32_t n_opts;
  const rm_options* opts;
  const uint32_t* trace_opt;  /* per trace index into opts */
} rm_batch_desc;

typedef struct {
  double threshold_sec;       /* reporter_service.py:55-58 (default 15) */
  uint32_t report_mask;       /* bit (level+1) set when level is reported; {0,1} = 0x6 */
  uint32_t transition_mask;
  uint32_t* hist_dev;         /* device pointer, n_segments*16 u32 speed histogram, may be NULL */
  int32_t do_report;          /* run the report() epilogue */
  int32_t zero_hist;          /* zero hist_dev (and dur_dev) on the runner's stream before the epilogue */
  uint64_t* dur_dev;          /* device pointer, n_segments u64: per OSMLR segment the sum of the reports'
                                 whole-second durations int(round(t1 - t0)) (the tile rows' duration
                                 column, py/simple_reporter.py:179) over the reports the histogram counts;
                                 may be NULL.  Integer sums, so the multi-GPU all-reduce is exact */
} rm_run_params;
void rm_default_run_params(rm_run_params* p);

/* upload + run every kernel; blocks until done */
int rm_runner_run(rm_runner* r, const rm_batch_desc* b, const rm_run_params* p);
/* run again over the batch already resident in HBM (bench steps) */
int rm_runner_rerun(rm_runner* r, const rm_run_params* p);
/* rerun n runners (contiguous parts of one batch, same engine) concurrently, one host thread
 * per part, so their kernels overlap on their streams; with zero_hist the shared histogram is
 * zeroed once before any part reports.  Returns the first part's error. */
int rm_runners_rerun(rm_runner* const* rs, uint32_t n, const rm_run_params* p);
/* out: [0] points [1] traces [2] transitions [3] path edges [4] segments [5] reports
 *      [6] route pairs sent to the wave tier [7] ... to the single-source tier
 *      [8] transitions sent to the path wave tier [9] states sent to the candidate wave tier */
int rm_runner_sizes(rm_runner* r, uint64_t out[10]);
/* K2 tier hand-overs of the last run: [0] items the ball tier passed to the search tiers,
 * [1] items the register search tier passed on, [2] items the second register tier passed on,
 * [3] chosen transitions the path ball tier passed to the path search tiers,
 * [4] route items the LDS wave tier passed to the global-memory tier, [5] likewise for paths,
 * [6] route items the 16-lane group tier passed to the 512-slot wave tier, [7] likewise for paths,
 * [8] route items the 512-slot wave tier passed to the 4096-slot one, [9] likewise for paths */
int rm_runner_route_tiers(rm_runner* r, uint64_t out[10]);
/* counters since the runner was created: [0] steady runs (large batches after the first, without
 * read-backs between the stages), [1] steady runs gated off on the device and run again the ordinary
 * way, [2] steady runs that did not launch the routes stage's hand-over tiers, [3] likewise the
 * path stage's */
int rm_runner_run_stats(rm_runner* r, uint64_t out[4]);
/* the steady scans' block bases on the host (test hook for rm_common.hpp scan_base_lane, which
 * engine.hip's BaseBuckets sums over an apply block's lanes): part
 * holds nb pairs of block partials, base receives nb pairs of exclusive prefixes, formed as a
 * block of `lanes` threads forms them from the coarse buckets and its group's partials */
int rm_scan_block_bases(const uint64_t* part, uint32_t nb, uint32_t lanes, uint64_t* base);
int rm_runner_get_states(rm_runner* r, uint32_t* n_states, uint32_t* state_orig);
int rm_runner_get_candidates(rm_runner* r, uint8_t* cand_n, uint32_t* road, uint32_t* s_cm, float* sq);
int rm_runner_get_routes(rm_runner* r, uint32_t* trans_off, double* gc, uint32_t* route_cm);
/* with turn costs (DESIGN.md §3 rule 3b): every transition's distance term turn_m + |route_m - gc|
 * in metres (+inf when invalid), as the Viterbi adds it; *present = 0 (nothing written) when no
 * trace of the last run had turn costs */
int rm_runner_get_route_terms(rm_runner* r, double* route_d, int* present);
int rm_runner_get_viterbi(rm_runner* r, int8_t* choice, uint8_t* chain_start);
int rm_runner_get_paths(rm_runner* r, uint32_t* path_off, uint32_t* path_cnt, uint32_t* path_edges, uint32_t* route_dist);
/* Matched points of the last run / rerun (DESIGN.md §3 rule 9): one 32-byte record per input
 * point, in batch point order (index trace_off[k] + q; n_points of rm_runner_sizes).  The stage
 * runs on this call, over what the run left in HBM (kernel id "points"); a run launches nothing
 * for it.  type 0 records (no chosen candidate at or before the point on its chain, or a trace
 * that failed under isolation) hold zeros except edge = 0xFFFFFFFF. */
typedef struct {
  float lon, lat;      /* snapped position */
  float sq;            /* squared distance in m^2 from the measurement to it (K1's local frame at the point) */
  uint32_t edge;       /* directed edge id, 0xFFFFFFFF when unmatched */
  uint32_t off_cm;     /* offset from the start of that directed edge */
  uint32_t way;        /* way id of the edge */
  uint32_t type;       /* 0 unmatched, 1 matched (a state with a chosen candidate), 2 interpolated */
  uint32_t route_cm;   /* distance along the transition's route from the previous state; 0 for type 1 */
} rm_matched_point;
int rm_runner_get_matched_points(rm_runner* r, rm_matched_point* out);
/* Matched edges of the last run / rerun (DESIGN.md §3 rule 10): one 64-byte record per edge visit
 * -- a maximal run of a chain's traversal records on one directed edge that join end to begin, as
 * the oracle's add_trav leaves them -- and one shape (f32 lon, lat pairs) per trace: per visit the
 * road position of its begin (a chain's first visit only), the road's stored vertices strictly
 * inside the part driven, in travel order, and the road position of its end.  A trace that failed
 * under isolation has no visits and an empty shape.
 * rm_runner_matched_edges runs the stage, over what the run left in HBM (a run launches nothing
 * for it; no kernel id: rm_runner_matched_edges_time gives the device time of the last call in
 * ms), and keeps the result on the device; out receives the visit count and the shape vertex
 * count of the batch.  rm_runner_get_matched_edges downloads that result: edge_off and shape_off
 * (n_traces + 1 each; trace k's visits are edges[edge_off[k] .. edge_off[k+1]), its vertices
 * shape[2 * shape_off[k] .. 2 * shape_off[k+1])), edges (out[0] records), shape (2 * out[1] floats). */
typedef struct {
  uint32_t edge, way;               /* directed edge id, its way id */
  uint32_t b_cm, e_cm;              /* the part driven, from the start of the directed edge */
  double t_enter, t_exit;           /* distance-interpolated epoch times at b_cm and e_cm */
  uint32_t begin_point, end_point;  /* point index within the trace of the state at / before either end */
  uint32_t shape_begin, shape_end;  /* first and last vertex of the visit in the trace's shape */
  uint32_t seg_dense, seg_off_cm;   /* dense OSMLR segment (0xFFFFFFFF: none), the edge's offset in it */
  uint32_t flags;                   /* bit 0 internal, bit 1 has an OSMLR segment, bit 2 first visit of its chain */
  uint32_t len_cm;                  /* length of the edge */
} rm_matched_edge;
int rm_runner_matched_edges(rm_runner* r, uint64_t out[2]);
int rm_runner_get_matched_edges(rm_runner* r, uint32_t* edge_off, rm_matched_edge* edges, uint32_t* shape_off, float* shape);
int rm_runner_matched_edges_time(rm_runner* r, double* ms);
/* segments: 56-byte records (rm::SegmentRec); seg_off has n_traces+1 entries */
int rm_runner_get_segments(rm_runner* r, uint32_t* seg_off, void* segs);
/* reports: 48-byte records (rm::ReportRec); stats: 40-byte rm::ReportStats per trace */
int rm_runner_get_reports(rm_runner* r, uint32_t* rep_off, void* reps, void* stats);
/* Failure isolation (default off: a trace that fails makes rm_runner_run return non-zero).
 * On: a trace that fails on its own — more than 192 roads inside its search radius, a route
 * search beyond every tier's capacity, a path that cannot be rebuilt — gets no segments and no
 * reports, the run succeeds for every other trace, and rm_runner_trace_errors gives the bits
 * (1 candidates, 2 route search, 8 path reconstruction) per trace.  The reference fails just
 * that request (py/reporter_service.py:244-245) or skips just that window
 * (py/simple_reporter.py:169-173). */
int rm_runner_set_isolation(rm_runner* r, int on);
int rm_runner_trace_errors(rm_runner* r, uint32_t* errs);   /* n_traces words of the last run */
/* Locality order of the stages that read regional graph data (K1 cell records, K2 route-ball
 * tables, the path walk): the state slots are sorted each step into the Morton-ordered cells of a
 * 64 x 64 grid over the graph (a counting sort) and those stages take their work in that order,
 * XCD-contiguously, so one region's tables meet in one L2.  mode 0: slot order; 1: K1 and K2 in
 * locality order; 2: the path stage too; -1 (default): 2 on graphs of >= 150 k nodes (env
 * RM_LOCALITY_NODES), 1 for batches sampled every >= 10 s on average on smaller graphs, else 0.
 * Env RM_LOCALITY sets the initial mode.  Results are identical in every mode.  *used: whether
 * the last run used it. */
int rm_runner_set_locality(rm_runner* r, int mode);
int rm_runner_locality_used(rm_runner* r, int* used);
/* per-kernel HIP-event timing on the runner's stream */
int rm_runner_set_timing(rm_runner* r, int on);
/* time only the stages whose bit is set (bit k = rm_kernel_name(k)): fewer event records in a timed region */
int rm_runner_set_timing_mask(rm_runner* r, uint32_t mask);
int rm_runner_kernel_times(rm_runner* r, double* ms, uint64_t* launches, int n);
int rm_runner_reset_times(rm_runner* r);
const char* rm_kernel_name(int k);
int rm_num_kernels(void);

/* ---------------- report() on host-supplied segment lists ----------------
 * The device report() epilogue (reference py/reporter_service.py:79-179) over segment lists
 * that did not come from the matcher: trace k's segments are segs[seg_off[k] .. seg_off[k+1])
 * (56-byte rm::SegmentRec), its last point's time trace_end_time[k] (:81), its threshold and
 * level masks per trace.  Reports come back compacted per trace (rep_off: n_traces+1 offsets,
 * reps: room for seg_off[n_traces] 48-byte records), stats: 40-byte rm::ReportStats per trace.
 * Uses the device of rm_set_device. */
typedef struct {
  uint32_t n_traces;
  const uint32_t* seg_off;
  const void* segs;
  const double* trace_end_time;
  const double* threshold_sec;
  const uint32_t* report_mask;      /* bit (level+1) per reported level */
  const uint32_t* transition_mask;
} rm_report_desc;
int rm_report_segments(const rm_report_desc* d, uint32_t* rep_off, void* reps, void* stats);
/* The same report() and then the complete /report reply of every trace (DESIGN.md section 3 rule 19):
 *   {"stats":{"successful_matches":{"count","length"},"unreported_matches":{"count","length"},
 *    "match_errors":{"discontinuities","invalid_speeds","invalid_times"},"unassociated_segments"}
 *    [,"shape_used"],"segment_matcher":{"segments":[...],"mode":"auto"},
 *    "datastore":{"mode":"auto","reports":[{"id","t0","t1","length","queue_length"[,"next_id"]}...]}}
 * with the segment objects of rm_match.  The n replies come in one malloc'd, NUL-terminated buffer
 * (rm_free): reply i is (*buf)[off[i], off[i+1]) (off: n_traces + 1 entries).  writer 1: the records
 * come down and the host formats them; 2: the text is written on the device from the records in HBM
 * and only text and offsets come down; 0: by size (2 above RM_REPLY_DEVICE_MIN_POINTS segments,
 * default 65536, read per call).  Both give the same bytes.  A trace holding a time that is
 * negative (other than -1), below 1 (other than 0), 2^53 or more or not finite is flagged: either
 * writer formats it on the host with std::to_chars.
 * info (may be NULL): [0] reply bytes [1] flagged traces [2] the writer used [3] the device writer's
 * kernels and scans in whole microseconds. */
int rm_report_replies(const rm_report_desc* d, int writer, char** buf, uint64_t* off, uint64_t info[4]);
/* The formatting alone, no GPU: trace k's segments are segs[seg_off[k] .. seg_off[k+1]) (56-byte
 * rm::SegmentRec), its reports reps[rep_off[k] .. rep_off[k+1]) (48-byte rm::ReportRec), stats
 * 40-byte rm::ReportStats per trace.  buf and off as above. */
int rm_report_format_host(uint32_t n, const uint32_t* seg_off, const void* segs, const uint32_t* rep_off,
                          const void* reps, const void* stats, char** buf, uint64_t* off);

/* ---------------- batch-pipeline stages around the matcher (reference py/simple_reporter.py) ----------------
 * rm_runner_run_points replaces the per-vehicle grouping, time sort and inactivity
 * windowing of simple_reporter.match (py/simple_reporter.py:137-164) with a device sort,
 * then matches every window of >= 2 points (as rm_runner_run).
 * rm_runner_tiles replaces the hour bucketing of the valid reports (:176-196) and the
 * report phase's sort, privacy cull and CSV (:211-254): it returns, per tile file,
 * "name\0body\0" where name is "<start>_<end>/<level>/<tile index>" and body the text
 * the reference uploads.  With a communicator the rows of every rank are all-gathered
 * and each rank returns the files it owns (file key hashed over ranks). */
typedef struct rm_comm rm_comm;
typedef struct {
  uint64_t n_points;
  const uint32_t* uuid;       /* dense vehicle index per point (< n_uuids) */
  const double* time;         /* epoch seconds (integers in the reference, :140) */
  const float* lon;
  const float* lat;
  const float* accuracy;      /* may be NULL */
  double inactivity_sec;      /* --inactivity, default 120 (:344) */
  uint32_t n_uuids;
  uint32_t n_opts;
  const rm_options* opts;
  const uint32_t* uuid_opt;   /* per vehicle index into opts; NULL = opts[0] for all */
} rm_points_desc;
int rm_runner_run_points(rm_runner* r, const rm_points_desc* d, const rm_run_params* p);
/* vehicle index of each matched window of the last rm_runner_run_points (n_traces entries) */
int rm_runner_get_trace_uuid(rm_runner* r, uint32_t* uuid);
/* the batch the last run matched: trace_off (n_traces+1), lon, lat, time, accuracy (n_points) */
int rm_runner_get_batch(rm_runner* r, uint32_t* trace_off, float* lon, float* lat, double* time, float* accuracy);
/* Trace-file text read on the device (DESIGN.md §3 rule 11): the parse half of the reference's
 * download phase (py/simple_reporter.py:100-113), the re-read of its match phase (:137-140) and
 * the streaming formatter's separated-value lines (Formatter.java:97-109).  One point per line,
 * fields split at `sep` (one byte, no quoting), columns counted from 0; acc_col -1: no accuracy
 * column (accuracy is then -1, absent).  time_format 0: decimal epoch seconds; 1: exactly 19 bytes
 * "YYYY-MM-DD HH:MM:SS" in UTC (digits at the fourteen digit positions).  accuracy_cap > 0: accuracy
 * is min(ceil(v), cap) (:112 uses 1000).  use_bbox: a point with lat < bbox[0] || lat > bbox[2] ||
 * lon < bbox[1] || lon > bbox[3] is dropped (:105).  rm_default_line_format: ',' and the columns
 * uuid 0, time 1, lat 2, lon 3, accuracy 4 of the trace files (:113), epoch seconds, no cap, no box. */
typedef struct { uint8_t sep; int32_t uuid_col, time_col, lat_col, lon_col, acc_col, time_format, accuracy_cap, use_bbox; double bbox[4]; } rm_line_format;
void rm_default_line_format(rm_line_format* f);
/* Date patterns (DESIGN.md §3 rule 18): the last argument of the reference's formatter string, a
 * Joda DateTimeFormat pattern such as yyyy-MM-dd'T'HH:mm:ssZZ, compiled once and read on the device.
 * rm_time_pattern compiles and registers a pattern: an id >= 16 to put into
 * rm_line_format.time_format, or -1 with the reason in err.  The same text gives the same id; at
 * most 240 patterns per process; thread-safe; ids are process-local (never stored in a snapshot).
 * time_format is 0, 1 or such an id: anything else fails the call that takes the format.  For
 * separated values a pattern whose literals hold the separator byte is a format error. */
int32_t rm_time_pattern(const char* pattern, char* err, size_t errlen);
/* the text of pattern `id` (NUL-terminated, cut to outlen): 0, or 1 when nobody registered the id */
int     rm_time_pattern_text(int32_t id, char* out, size_t outlen);
/* host only: one text under one pattern -> 0 and *seconds, 1 (malformed), or 2 (no such id) */
int     rm_time_pattern_parse(int32_t id, const char* text, size_t n, double* seconds);
/* The input: n_chunks byte ranges (one per file; a chunk without a final newline ends its last
 * line), under 2^32 bytes together.  Every window takes opts[0]. */
typedef struct { uint32_t n_chunks; const char* const* data; const uint64_t* len; rm_line_format fmt;
                 double inactivity_sec; uint32_t n_opts; const rm_options* opts; } rm_lines_desc;
/* A malformed line fails either call with "chunk <c> line <l>: <reason>" (both 1-based, the first
 * bad line in input order).  Vehicle ids are numbered in first-seen order over the kept points. */
int rm_runner_run_lines(rm_runner* r, const rm_lines_desc* d, const rm_run_params* p);   /* parse, ids, windows, match */
int rm_runner_parse_lines(rm_runner* r, const rm_lines_desc* d);                          /* parse and ids only */
/* out: lines, blank, outside the box, points, vehicles, lines read on the host, 1 when the ids were assigned on the host */
int rm_runner_lines_info(rm_runner* r, uint64_t out[7]);
int rm_runner_get_line_points(rm_runner* r, uint32_t* uuid, double* time, float* lon, float* lat, float* acc); /* input order */
int rm_runner_get_vehicles(rm_runner* r, uint32_t* chunk, uint64_t* off, uint32_t* len);   /* name span per vehicle */
int rm_runner_lines_time(rm_runner* r, double ms[4]);   /* upload, parse (+ host lines), ids, windows */
/* host only, no GPU: the generic rule over the same input; arrays sized by a first call with NULLs */
int rm_lines_parse_host(const rm_lines_desc* d, uint64_t info[7], uint32_t* uuid, double* time, float* lon, float* lat,
                        float* acc, uint32_t* chunk, uint64_t* off, uint32_t* len, char* err, size_t errlen);
/* Gzip input (DESIGN.md §3 rule 20): the reference's source files are gzip (load_data.sh:11,
 * simple_reporter.py:99).  A chunk is a sequence of gzip members read as Python's gzip module reads
 * them: FEXTRA / FNAME / FCOMMENT / FHCRC skipped (the FHCRC value and the reserved flag bits are
 * not checked, unlike zlib's gzread), CRC-32 and ISIZE checked per member, zero bytes after a
 * trailer skipped, the window not carried across members.  status[c]: 0 ok, 1 header, 2 truncated,
 * 3 malformed block, 4 CRC, 5 size, 6 too large: the first error in stream order.  out_len[c]: the
 * chunk's inflated bytes (0 for a bad chunk); *blob (library-allocated, rm_free): the good chunks'
 * bytes end to end in input order.  The call itself fails only for NULL arguments, a device error,
 * or more than 2^32 inflated bytes.  rm_inflate decodes one chunk per wave on `device`;
 * rm_inflate_host runs the same decoder core on the host pool, no GPU.  rm_inflate_last: of the
 * calling thread's last rm_inflate / rm_inflate_host (either may be NULL) info: members, bytes in,
 * bytes out, chunks that took the device's second pass (their slot, sized from the last member's
 * ISIZE, was too small); ms: device inflate (with the CRC, which is computed as the window is
 * flushed), 0, gather. */
int rm_inflate(int device, uint32_t n, const char* const* data, const uint64_t* len, uint32_t* status,
               uint64_t* out_len, char** blob, size_t* blob_len);
int rm_inflate_host(uint32_t n, const char* const* data, const uint64_t* len, uint32_t* status,
                    uint64_t* out_len, char** blob, size_t* blob_len);
void rm_inflate_last(uint64_t info[4], double ms[3]);
const char* rm_inflate_status_text(uint32_t status);
/* The runner's input coding, sticky: how rm_runner_run_lines, rm_runner_parse_lines and
 * rm_session_push_messages* read their chunks from now on.  0 plain (the default: bytes are text
 * whatever they look like), 1 gzip (every chunk), 2 gzip where a chunk begins 1f 8b.  Gzip chunks are
 * inflated on the device into the text the line reader parses, so line numbers, lines_info and the
 * points cannot tell the difference; a call with fewer than RM_INFLATE_DEVICE_MIN_CHUNKS gzip chunks
 * (environment; default 1024, the measured break-even: DESIGN.md §5) inflates them on the host pool with the same decoder core and uploads
 * plain text.  A bad chunk fails the call with "chunk <c>: gzip: <reason>" (the first in input order);
 * with skip_bad it counts as empty and its status stays readable (the reference logs and skips the
 * file, simple_reporter.py:128-129).  The 2^32 byte limit of a call applies to the inflated total.
 * rm_runner_get_vehicles' spans then refer to inflated text the caller does not hold:
 * rm_runner_get_text reads bytes [off, off + len) of chunk `chunk` of the last parse back from the
 * device (any coding).
 * chunk_count: the chunks of the runner's last parse, whichever call made it (a push included);
 * chunk_status: that many words (0 for plain chunks).
 * inflate_info: chunks inflated, members, bytes in, bytes out, second-pass chunks, chunks inflated on
 * the host.  inflate_time: inflate (with the CRC), 0, gather; the compressed upload is part of
 * rm_runner_lines_time's "upload". */
int rm_runner_set_input_coding(rm_runner* r, int coding, int skip_bad);
int rm_runner_chunk_count(rm_runner* r, uint32_t* n);
int rm_runner_chunk_status(rm_runner* r, uint32_t* status);
int rm_runner_inflate_info(rm_runner* r, uint64_t out[6]);
int rm_runner_inflate_time(rm_runner* r, double ms[3]);
int rm_runner_get_text(rm_runner* r, uint32_t chunk, uint64_t off, uint64_t len, char* out);
typedef struct {
  uint32_t quantisation;      /* --quantisation, default 3600 (:343) */
  uint32_t privacy;           /* --privacy, default 2 (:345) */
  const char* source;         /* --source-id, default "smpl_rprt" (:346) */
  const char* mode;           /* vehicle type column, upper-cased (:194) */
} rm_tile_params;
void rm_default_tile_params(rm_tile_params* p);
/* blob is library-allocated (free with rm_free); comm may be NULL */
int rm_runner_tiles(rm_runner* r, const rm_tile_params* p, rm_comm* comm, char** blob, size_t* len);

/* ---------------- vehicle sessions (reference BatchingProcessor.java, Batch.java) ----------------
 * The streaming topology's batcher kept in HBM beside a runner (DESIGN.md §3 rule 12): per vehicle
 * the points in arrival order, the running maximum distance from the first point and the stream
 * time of the last arrival.  rm_session_push appends a micro-batch of arrivals and, wherever the
 * reference's rule triggers (>= report_dist_m from the first point, >= report_count points,
 * >= report_time_s between the first and the last), matches the vehicle's list as one trace on the
 * runner, runs report() over it, trims the list to shape_used (clears it when the reply has none,
 * or when the match failed) and searches on; rm_session_punctuate evicts the vehicles whose last
 * arrival is more than session_gap_ms old, reporting what they hold with thresholds (0, 2, 0).
 * The forwarded reports of a call (Segment.valid(), Segment.java:38-40) come back ordered by the
 * arrival that triggered them, so the same arrivals cut into pushes of any sizes give the same
 * concatenated output.  The runner's batch is replaced by each round's windows; one runner serves
 * one session at a time (the session keeps what it needs of the runner alive, so either may be
 * destroyed first).  run.do_report is forced on and run.zero_hist off: hist_dev / dur_dev
 * accumulate over the calls. */
typedef struct rm_session rm_session;
typedef struct {
  double report_dist_m;          /* 500 (BatchingProcessor.java:28) */
  uint32_t report_count;         /* 10  (:27) */
  uint32_t max_vehicle_points;   /* 0: unbounded, as the reference; above 0, a list that reaches it on an
                                    arrival that does not trigger is cleared (a window record with err
                                    0x80000000 and no match) */
  double report_time_s;          /* 60  (:26) */
  int64_t session_gap_ms;        /* 60000 (:29) */
  rm_options opt;                /* one option set for every vehicle (Batch.java:58-60) */
  rm_run_params run;             /* threshold, level masks, hist_dev / dur_dev */
} rm_session_params;
void rm_default_session_params(rm_session_params* p);
typedef struct {
  uint64_t n;
  const uint32_t* vehicle;       /* dense vehicle index per arrival (< n_vehicles) */
  const double* time;            /* epoch seconds */
  const float* lon;
  const float* lat;
  const float* accuracy;         /* may be NULL: absent (-1) */
  const int64_t* stamp_ms;       /* stream time of each arrival (context.timestamp()) */
} rm_session_points;
typedef struct {                 /* rm::ReportRec and where it came from */
  uint64_t id, next_id;
  double t0, t1;
  int32_t length, queue_length;
  uint32_t seg_dense, pad;
  uint32_t vehicle, window;      /* window: index into the same call's rm_session_get_windows */
} rm_session_report;
typedef struct {
  uint32_t vehicle;
  uint32_t arrival;              /* index in the push of the arrival that triggered (punctuate: the vehicle) */
  uint32_t n_points;
  int32_t shape_used;            /* -1 when absent */
  uint32_t n_reports;            /* before the forwarding filter */
  uint32_t err;                  /* the window's error bits (rm_runner_trace_errors); 0x80000000: cleared at
                                    max_vehicle_points */
} rm_session_window;
rm_session* rm_session_create(rm_runner* r, uint32_t n_vehicles, const rm_session_params* p);   /* NULL on error */
void rm_session_destroy(rm_session* s);
/* out: [0] arrivals evaluated (those that found a list to join) [1] triggers [2] trims (shape_used
 * present) [3] lists cleared by an absent shape_used [4] failed windows [5] forwarded reports
 * [6] invalid reports [7] match rounds.  A vehicle index out of range or a NaN time fails the call
 * and leaves the session as it was. */
int rm_session_push(rm_session* s, const rm_session_points* pts, uint64_t out[8]);
int rm_session_punctuate(rm_session* s, int64_t timestamp_ms, uint64_t out[8]);
/* The last call's forwarded reports / window records, ordered by triggering arrival (reports in
 * report() order inside a window).  *n receives the count; out may be NULL (count only). */
int rm_session_get_reports(rm_session* s, rm_session_report* out, uint64_t* n);
int rm_session_get_windows(rm_session* s, rm_session_window* out, uint64_t* n);
/* The store: per vehicle cnt, max_sep, last_update (n_vehicles each; the latter two are 0 for an
 * empty vehicle) and the kept points packed in vehicle order (*n_points of them).  Any array may
 * be NULL. */
int rm_session_get_store(rm_session* s, uint32_t* cnt, float* max_sep, int64_t* last_update, float* lon, float* lat,
                         double* time, float* accuracy, uint64_t* n_points);
/* device time (ms, HIP events) of the last call: upload, append, trigger, match, trim */
int rm_session_time(rm_session* s, double ms[5]);

/* ---------------- stream messages (reference KeyedFormattingProcessor.java, Formatter.java) ----------------
 * The streaming topology's first processor on the device (DESIGN.md §3 rule 14): raw messages, one
 * per line, become vehicle keys and points and go into a session without leaving HBM.
 * kind 0: separated values, `line` as rm_runner_parse_lines reads it.  kind 1: one JSON object per
 * line; of `line` the time_format, accuracy_cap, use_bbox and bbox apply; key[0..4] name the id,
 * lat, lon, time and accuracy members (NUL-terminated, at most 31 bytes, no '"', '\' or byte below
 * 0x20, all different; an empty accuracy key: no accuracy, the value is -1).  lat, lon and accuracy
 * are numbers or strings holding one, the time (format 0) an integer number or string, (format 1)
 * a 19-byte string, the id a string without an escape or an integer number token. */
typedef struct { int32_t kind; int32_t pad; rm_line_format line; char key[5][32]; } rm_message_format;
void rm_default_message_format(rm_message_format* f);   /* kind 0, the default line format, the keys
                                                           id, latitude, longitude, timestamp, accuracy */
/* chunks as in rm_lines_desc.  strict 1: the first malformed message in input order fails the call
 * with "chunk <c> line <l>: <reason>"; 0 (the stream's behaviour, KeyedFormattingProcessor.java:33-41):
 * it is dropped and counted.  has_stamp 1: every message carries stamp_ms as its stream time; 0: each
 * carries (int64)(time * 1000) of its own. */
typedef struct { uint32_t n_chunks; const char* const* data; const uint64_t* len; rm_message_format fmt;
                 int32_t strict; int32_t has_stamp; int64_t stamp_ms; } rm_messages_desc;
/* The vehicle directory: id bytes -> a dense index that holds for the whole stream, first-seen
 * order over the kept points of all calls, kept in HBM.  NULL on error. */
typedef struct rm_directory rm_directory;
rm_directory* rm_directory_create(int device, uint32_t max_vehicles);
void rm_directory_destroy(rm_directory* d);
int rm_directory_size(rm_directory* d, uint32_t* n);
/* vehicles [first, first + n): off (n + 1 entries, from 0) into bytes; either may be NULL;
 * *n_bytes receives the bytes of the range (a first call sizes `bytes`) */
int rm_directory_names(rm_directory* d, uint32_t first, uint32_t n, uint64_t* off, char* bytes, uint64_t* n_bytes);
/* Upload the text, read the messages, number the vehicles through the directory and push the
 * points into the session, all on the session's GPU.  out: as rm_session_push.  info: as
 * rm_runner_lines_info ([4]: the call's distinct vehicles), then [7] the dropped messages.  The
 * directory's max_vehicles must not exceed the session's n_vehicles, and both must be on one
 * device.  A malformed message of a strict call, a call that would pass max_vehicles ("directory
 * full") and one whose points do not fit the session's store fail before anything is written and
 * leave the directory and the session as they were.  A failure behind the keying (a HIP error, or
 * HBM running out while the session appends) leaves the session as rm_session_push does and the
 * call's new ids in the directory: they keep their indices when the messages are sent again. */
int rm_session_push_messages(rm_session* s, rm_directory* dir, const rm_messages_desc* d, uint64_t out[8], uint64_t info[8]);
/* the first (at most 64) dropped messages of the last rm_session_push_messages, in input order:
 * chunk and line (1-based), and the reasons as NUL-terminated strings laid end to end in `reasons`
 * (reasons_len bytes; 64 * 64 suffice).  *n receives how many are listed. */
int rm_session_dropped_messages(rm_session* s, uint32_t* n, uint32_t chunk[64], uint64_t line[64], char* reasons, size_t reasons_len);
/* host only, no GPU: the generic rule over the same input, vehicles numbered per call; arrays sized
 * by a first call with NULLs (info[3] points, info[4] vehicles); drop_* as rm_session_dropped_messages */
int rm_messages_parse_host(const rm_messages_desc* d, uint64_t info[8], uint32_t* uuid, double* time, float* lon, float* lat,
                           float* acc, uint32_t* chunk, uint64_t* off, uint32_t* len, uint32_t* n_drop, uint32_t drop_chunk[64],
                           uint64_t drop_line[64], char* reasons, size_t reasons_len, char* err, size_t errlen);
/* the smallest and the largest time (epoch seconds) among the points the last
 * rm_session_push_messages kept; *n_points 0: none, t is not written */
int rm_session_messages_span(rm_session* s, double t[2], uint64_t* n_points);
/* device time (ms, HIP events) of the last rm_session_push_messages: upload, parse (+ host lines),
 * ids, directory, then rm_session_time's five */
int rm_session_messages_time(rm_session* s, double ms[9]);

/* ---------------- tile store (reference AnonymisingProcessor.java, TimeQuantisedTile.java) ----------------
 * The streaming topology's anonymiser kept in HBM (DESIGN.md §3 rule 13).  rm_tilestore_add is
 * process(): every segment that passes Segment.valid() adds one row to each time-quantised tile
 * (trunc(t0) / quantisation .. trunc(t1) / quantisation, id & 0x1FFFFFF) it touches, in arrival
 * order; rm_tilestore_add_session takes a session's forwarded reports straight from its device
 * buffer.  rm_tilestore_flush is punctuate(): every tile sorted stably by (id, next_id) as
 * integers, culled by clean() with the privacy count, and written as the CSV body the datastore
 * ingests -- sort, cull and text on the GPU -- after which the store is empty.  The blob holds
 * "name\0body\0" per file, files ordered by (time range start, tile id); name is
 * "<start>_<start + quantisation - 1>/<level>/<tile index>", body the column header and one
 * "\n"-led row per segment (no trailing newline).  The random file name under the tile directory
 * and the sinks stay with the caller.  A store has its own stream and serves one calling thread at
 * a time; it may be fed from any number of sessions on its device, one call after another.
 * Stated limits: an id or next_id above 2^63 - 1, a non-finite time or t1 >= 2^53, or a segment
 * spanning more than 65,536 buckets fails the add call and leaves the store as it was; a source
 * longer than 64 bytes, a mode longer than 16, or either with ',' or a newline fails creation, as
 * do quantisation < 60 and privacy < 1 (AnonymisingProcessor.java:73-80). */
typedef struct rm_tilestore rm_tilestore;
typedef struct { uint64_t id, next_id; double t0, t1; int32_t length, queue_length; } rm_tile_segment;
rm_tilestore* rm_tilestore_create(int device, const rm_tile_params* p, uint64_t initial_rows);   /* NULL on error */
void rm_tilestore_destroy(rm_tilestore* t);
/* out: [0] segments kept [1] segments skipped as !valid() [2] rows appended [3] rows held */
int rm_tilestore_add(rm_tilestore* t, const rm_tile_segment* segs, uint64_t n, uint64_t out[4]);
/* the session's last push / punctuate; a session on another device than the store fails */
int rm_tilestore_add_session(rm_tilestore* t, rm_session* s, uint64_t out[4]);
/* blob is library-allocated (free with rm_free).
 * out: [0] rows in [1] rows kept [2] tiles held [3] files written [4] blob bytes */
int rm_tilestore_flush(rm_tilestore* t, char** blob, size_t* len, uint64_t out[5]);
/* device time (ms, HIP events) of the last call: upload, expand, sort, cull, text, download */
int rm_tilestore_time(rm_tilestore* t, double ms[6]);

/* ---------------- stream snapshot (DESIGN.md §3 rule 15) ----------------
 * The state of a stream -- every vehicle's open point list (rm_session), every id-to-index
 * assignment (rm_directory), every tile row still waiting for its privacy count (rm_tilestore) --
 * saved into one versioned, checksummed blob and restored from it: the reference's changelog-backed
 * state stores (BatchingProcessor.GetStore, AnonymisingProcessor.GetTileStore / GetMapStore).  A
 * stream stopped anywhere, saved, torn down, rebuilt from the blob and continued gives the output of
 * the stream that never stopped, bit for bit.
 *
 * Any of the three objects may be NULL: a save leaves that section out, a load skips it.  A load
 * into an object whose section is absent fails, as do objects on different devices.  The targets of
 * a load must be empty, as created; the blob's sessions fit any n_vehicles above the largest saved
 * index and its names any max_vehicles and any RM_LINES_HASH_BITS (the table is rebuilt).  A load
 * that fails -- a damaged or forged blob (each clause of the rule has its own message), a target too
 * small, a quantisation other than the tile store's, HBM running out -- leaves its targets empty and
 * usable.  A save changes nothing the stream will output.
 *
 * What is not state: the session's thresholds, options and run parameters, the tile store's source,
 * mode and privacy (they are the loading objects'); the last call's windows and reports (after a load
 * rm_session_get_reports gives 0 and rm_tilestore_add_session adds nothing); and the run parameters'
 * hist_dev / dur_dev, which belong to the caller and are not part of a snapshot.
 *
 * save: *blob is library-allocated (free with rm_free); `user` bytes travel opaque.
 *   out: [0] blob bytes [1] names [2] vehicles holding points [3] points [4] tile rows [5] user bytes
 *   ms (HIP events): [0] pack [1] gather [2] checksum [3] download
 * load: out as for save; ms: [0] upload [1] check [2] unpack */
int rm_snapshot_save(rm_session* s, rm_directory* d, rm_tilestore* t, const char* user, size_t user_len, char** blob,
                     size_t* len, uint64_t out[6], double ms[6]);
int rm_snapshot_load(rm_session* s, rm_directory* d, rm_tilestore* t, const char* blob, size_t len, uint64_t out[6],
                     double ms[6]);
/* Host only, no GPU: header, table, checksums and the whole structural rule that does not need the
 * loading objects.  info: [0] version [1] bytes [2] names [3] vehicles [4] points [5] rows
 * [6] quantisation [7] user offset [8] user bytes.  On failure the reason is in err (and rm_last_error). */
int rm_snapshot_check_host(const char* blob, size_t len, uint64_t info[9], char* err, size_t errlen);

/* ---------------- RCCL over xGMI (multi-GPU histogram exchange) ----------------
 * One process per GPU.  Replaces the reference's keyed Kafka repartition of
 * "id next_id" reports (BatchingProcessor.java:126) with one all-reduce of the
 * per-OSMLR-segment speed histogram.  Rank 0 creates the id, every rank inits. */
int rm_comm_unique_id(uint8_t id_out[128]);
rm_comm* rm_comm_init(int nranks, int rank, const uint8_t id[128], int device);
void rm_comm_destroy(rm_comm* c);
/* dtype: 0 u32, 1 u64, 2 f64; op: 0 sum, 1 max.  In place on a device buffer (a host buffer on a
 * device -1 host-transport communicator); blocks until done. */
int rm_comm_allreduce(rm_comm* c, void* dev_buf, size_t count, int dtype, int op);
/* The optional exchange of SURVEY §8(e): each rank owns one segment-id range.  buf holds nranks
 * chunks of count_per_rank elements; on return chunk `rank` holds the reduction of every rank's
 * chunk `rank` (RCCL reduce-scatter, in place), the other chunks are unspecified.  Half the bytes
 * per rank of an all-reduce; buffers as rm_comm_allreduce.  For the speed histogram (16 bins per
 * segment) count_per_rank must be 16 x the segments per rank, so no segment's bins are split. */
int rm_comm_reduce_scatter(rm_comm* c, void* buf, size_t count_per_rank, int dtype, int op);
/* all-reduce of one host double (op as above) */
int rm_comm_allreduce_host_f64(rm_comm* c, double* value, int op);
int rm_comm_barrier(rm_comm* c);
/* A communicator over a host transport the caller supplies (e.g. the gloo backend of an
 * existing job, or a test harness): fn must be a blocking all-gather across the nranks callers,
 * placing every rank's `bytes` bytes of send at recv + rank * bytes, and return 0.  Every rm_comm
 * operation then runs over it (device buffers staged through host memory); device -1 makes a
 * host-only communicator (rm_comm_allreduce_host_f64 and rm_comm_barrier work without a GPU). */
typedef int (*rm_host_allgather_fn)(void* ctx, const void* send, size_t bytes, void* recv);
rm_comm* rm_comm_init_host(int nranks, int rank, rm_host_allgather_fn fn, void* ctx, int device);
/* Host-only: the rank that culls and writes time-tile file (bucket, level | tile index << 3) when
 * rm_runner_tiles runs with an nranks communicator (the device filter uses the same function). */
int rm_tile_file_owner(uint64_t bucket, uint32_t tile, int nranks);

/* ---------------- the stream on several GPUs (DESIGN.md §3 rule 16) ----------------
 * A stream of nranks ranks gives, file for file and byte for byte, the output of the one-rank stream
 * over the same polls, and each file is written by exactly one rank.  Every rank makes the same
 * calls on the same text (reading and keying are replicated, so the directories agree index for
 * index); the sessions are sharded by vehicle, rm_vehicle_owner(directory index, nranks): a
 * multiplicative hash, so first-seen order does not stripe the load; and just before a flush the
 * tile rows go to the rank rm_tile_file_owner names for their file.
 *
 * rm_session_push_messages_sharded reads, keys and drops exactly as rm_session_push_messages (info,
 * the dropped list and rm_session_messages_span are the same on every rank), then appends, triggers
 * and matches only the points of the vehicles `rank` owns.  A window's arrival stays the index among
 * all kept points of the call.  shard: [0] own points [1] foreign points.  rm_session_punctuate
 * needs no change.
 *
 * A tile store numbers its add calls from 0 and keeps, beside every row, key = call << 32 | a: the
 * triggering arrival of the row's report (rm_tilestore_add_session), the segment's index in the
 * array (rm_tilestore_add).  Keys are kept from the store's first call below, or its first
 * rm_tilestore_add_session of a session that was pushed sharded; a store that sees neither
 * allocates and launches nothing for them.  (Rows added before that from a session never pushed
 * sharded get their report's index for a: rows of one rank in that rank's order.)
 *   rm_tilestore_export_rows   the rows held and their keys as a library-allocated blob (rm_free);
 *                              the store keeps them
 *   rm_tilestore_import_owned  clears the store and loads, of the n blobs (in rank order), the rows
 *                              whose file `rank` owns, merged by one stable sort on the key -- the
 *                              one-rank store's order exactly, so rm_tilestore_flush runs unchanged
 *   rm_tilestore_exchange      export -> all-gather -> import on the device through `comm` (RCCL or
 *                              the host transport; every rank calls it, padded to the largest count)
 *   out: [0] rows before [1] rows sent away [2] rows received [3] rows held
 *   rm_tilestore_exchange_time ms (HIP events) of the last import / exchange: partition, transport, merge
 * Not supported: ranks reading disjoint parts of the input, which would need order keys taken from
 * the messages themselves.  A sharded stream is saved and restored by the calls of rule 17 below:
 * rm_snapshot_save of a store that keeps keys, and rm_snapshot_load into one, still fail with a
 * message (rows restored by rm_snapshot_load cannot be exported either). */
int rm_vehicle_owner(uint32_t index, int nranks);
int rm_session_push_messages_sharded(rm_session* s, rm_directory* dir, const rm_messages_desc* d, int nranks, int rank,
                                     uint64_t out[8], uint64_t info[8], uint64_t shard[2]);
int rm_tilestore_export_rows(rm_tilestore* t, char** blob, size_t* len);
int rm_tilestore_import_owned(rm_tilestore* t, const char* const* blobs, const size_t* lens, uint32_t n, int nranks, int rank,
                              uint64_t out[4]);
int rm_tilestore_exchange(rm_tilestore* t, rm_comm* comm, uint64_t out[4]);
int rm_tilestore_exchange_time(rm_tilestore* t, double ms[3]);

/* ---------------- checkpoints of the stream on several GPUs (DESIGN.md §3 rule 17) ----------------
 * A stream of M ranks stopped behind any poll, saved rank by rank, torn down, rebuilt on N ranks from
 * the M blobs and continued writes, file for file and byte for byte, what the one-rank stream that
 * never stopped writes; M and N are each 1 .. 16 and need not be equal (the reference's changelog
 * restore and rebalance).  A blob of this kind is a snapshot blob (version 1) with two more sections:
 * kind 11, the u64 key of every tile row, and kind 12, one record {u32 rank, nranks, calls, 0}.
 *
 * rm_snapshot_save_shard   rank's blob: its sessions, the directory (replicated), its rows, their keys
 *                          and the record; the store is needed and keeps keys from here on.  out and
 *                          ms as for rm_snapshot_save.
 * rm_snapshot_load_shards  into empty objects, from the n_blobs blobs of one save in any order: the
 *                          sessions of the vehicles rm_vehicle_owner gives to `rank` of `nranks`, the
 *                          directory, and the rows of the files rm_tile_file_owner gives it, in the
 *                          one-rank order.  The blobs must be all M of one save (their nranks is
 *                          n_blobs, every rank once, equal calls, equal directories) and of the
 *                          store's quantisation.  One blob without kinds 11 and 12 (rm_snapshot_save's)
 *                          counts as rank 0 of 1: its rows are keyed by position under call 0.  The
 *                          session counts as pushed sharded afterwards and the store keeps keys.  A
 *                          load that fails leaves its targets empty and usable.
 *   out: [0] bytes of all blobs [1] names [2] vehicles held [3] points held [4] rows held
 *        [5] user bytes of the first blob [6] calls [7] saved ranks
 *   ms (HIP events): [0] upload [1] check [2] unpack [3] the rows' partition and merge
 * rm_snapshot_load refuses a blob with kinds 11 and 12, naming rm_snapshot_load_shards.
 * rm_snapshot_check_host_shard is rm_snapshot_check_host with three more words:
 *   info: [9] rank [10] nranks (0: no shard record) [11] calls */
int rm_snapshot_save_shard(rm_session* s, rm_directory* d, rm_tilestore* t, int rank, int nranks, const char* user,
                           size_t user_len, char** blob, size_t* len, uint64_t out[6], double ms[6]);
int rm_snapshot_load_shards(rm_session* s, rm_directory* d, rm_tilestore* t, const char* const* blobs, const size_t* lens,
                            uint32_t n_blobs, int rank, int nranks, uint64_t out[8], double ms[6]);
int rm_snapshot_check_host_shard(const char* blob, size_t len, uint64_t info[12], char* err, size_t errlen);

/* ---------------- device memory helpers (histograms without a framework) ---------------- */
int rm_device_alloc(size_t bytes, void** dev_ptr);
int rm_device_free(void* dev_ptr);
int rm_device_memset(void* dev_ptr, int value, size_t bytes);
int rm_device_download(void* host_dst, const void* dev_src, size_t bytes);
int rm_device_upload(void* dev_dst, const void* host_src, size_t bytes);
int rm_device_synchronize(void);

#ifdef __cplusplus
}
#endif
#endif
