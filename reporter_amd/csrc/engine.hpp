// engine.hpp — MI355X map-matching engine: the graph resident in HBM and the
// per-batch device workspace that the gfx950 kernels (engine.hip) run over.
//
// One Engine per process/GPU holds the read-only graph.  Each Matcher (one per
// calling thread, the threading contract of reference py/reporter_service.py:28-64)
// owns a HIP stream and a grow-only Workspace, so distinct matchers run
// concurrently without sharing mutable device state.
#pragma once
#include <hip/hip_runtime.h>

#include <functional>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "balls.hpp"
#include "dev_util.hpp"
#include "graph.hpp"
#include "rm_common.hpp"
#include "msg_lines.hpp"
#include "serve_policy.hpp"
#include "sv_lines.hpp"

namespace rm {

struct DevGraph {  // POD view of the graph in HBM, passed by value to kernels
  const uint32_t* node_off;
  const uint4* edges;            // EdgeRec
  const uint32_t* edge_src;      // source node of each directed edge
  const uint32_t* in_off;        // in-edge CSR offsets (N+1)
  const uint32_t* in_edge;       // edge ids by target node, ascending
  const uint4* in_rec;           // per in-edge: {edge, source node, road << 1 | rev, len_cm}
  const uint32_t* in_info;       // per in-edge: the edge's info word
  const uint32_t* edge_seg;
  const uint32_t* edge_seg_off;
  const uint32_t* edge_way;
  const uint32_t* road_node0;
  const uint32_t* road_node1;
  const uint32_t* road_fwd;
  const uint32_t* road_rev;
  const uint32_t* road_len;
  const uint4* verts;            // VertRec
  const unsigned long long* seg_id;
  const uint32_t* seg_len;
  const uint32_t* cell_off;
  const uint32_t* cell_item;
  const uint4* cell_rec;         // per cell item, 2 x uint4: {A.lon, A.lat, B.lon, B.lat}, {A.cum, B.cum, road | acc << 29, vertex}
  const uint4* road_rec;         // per road, 2 x uint4: {node0, node1, len_cm, fwd edge}, {rev edge, info fwd, info rev, 0}
  const uint4* relax[5];         // per travel mode, per directed edge: {target, len_cm | 0xffffffff if the mode
                                 // cannot use it, time_ms at the mode's speed, CSR range of the target}
  const uint32_t* node_rng;      // per node: first out-edge << 5 | out-degree
  const uint4* seg_rec;          // per directed edge, for K4: {len_cm | reversed << 31 | internal << 30, segment, offset, way}
  // route balls per travel mode (balls.hpp): per node {first entry, log2 table size or 0},
  // entries {node | kNone, dist cm, time ms, 0}; radius 0 = not built (K2 searches instead)
  const uint2* ball_hdr[5];
  const uint4* ball_ent[5];
  uint32_t ball_radius[5];
  uint32_t ball_mask;            // modes whose balls are built
  uint32_t ball_road_mask;       // road-id bits of a row's first word (rm_common.hpp ball_road_mask)
  // turn costs (rule 3b): per road its two headings (rm_common.hpp head_start / head_back), the
  // turn weight of each turn degree 0..180, and per mode the turn rows parallel to ball_ent
  // ({node0 word, node1 word} per slot: the turn weight of the canonical route from the table's
  // node to the road's endpoint, entering the road there, without the turn at the table's node
  // | the heading the route leaves that node with << 23; k_ball_turns)
  const uint32_t* road_head;
  const uint32_t* turn_w;
  const uint2* ball_turn[5];
  uint32_t ball_turn_mask;       // modes whose turn rows are built
  double lon0, lat0, dlon, dlat;
  uint32_t ncx, ncy, n_nodes, n_edges, n_segments, pad;
};

// Host-side description of one batch of traces (arrays live in host memory).
struct HostBatch {
  uint32_t n_traces = 0;
  const uint32_t* trace_off = nullptr;  // n_traces + 1
  const float* lon = nullptr;
  const float* lat = nullptr;
  const double* time = nullptr;
  const float* accuracy = nullptr;      // < 0 when absent
  uint32_t n_opts = 0;
  const MatchOptions* opts = nullptr;
  const uint32_t* trace_opt = nullptr;  // per trace
};

struct RunParams {
  double threshold_sec = 15.0;          // reporter_service.py:55-58
  uint32_t report_mask = 0b0110;        // levels {0,1}: bit (level+1)
  uint32_t transition_mask = 0b0110;
  uint32_t* hist = nullptr;             // device, n_segments * 16 u32 (may be null)
  int do_report = 1;
  int zero_hist = 0;                    // memset hist (and dur) on the stream before the epilogue
  unsigned long long* dur = nullptr;    // device, n_segments u64 duration sums in whole seconds (may be null)
  // a small batch (Matcher::run_small) also lays out and compacts its segments on the device
  // before its one read-back, so get_segments is a single copy (the service's reply path)
  int prefetch_segments = 0;
  // A Report run (DESIGN.md §3 rule 19): the level masks per trace (host arrays of n_traces words,
  // both or neither; null: the two scalars above for every trace) ...
  const uint32_t* trace_report_mask = nullptr;
  const uint32_t* trace_transition_mask = nullptr;
  // ... and a small run also readies its reports and stats for its one read-back (prefetch_segments)
  int prefetch_reports = 0;
};

// Device addresses of a batch's inputs: the workspace's arrays, or (a small run()) the one
// block its single upload filled
struct InputView {
  const uint32_t* trace_off = nullptr;
  const float* lon = nullptr;
  const float* lat = nullptr;
  const double* time = nullptr;
  const float* acc = nullptr;
  const MatchOptions* opts = nullptr;
  const uint32_t* trace_opt = nullptr;
};

// Kernel ids for per-kernel HIP-event timing.
enum KernelId { kKStates = 0, kKCandidates, kKScan, kKRoutes, kKViterbi, kKPaths, kKSegments, kKReport, kKLocality,
                kKPoints, kNumKernels };
extern const char* const kKernelNames[kNumKernels];

// Device workspace of one batch.  All arrays are indexed by point slot p
// (state s of trace k lives at slot trace_off[k] + s).
constexpr int kCtlWords = 16;
// The control words (Workspace::ctl, zeroed by k_states; Matcher::ctl_words returns them in this
// order).  A hand-over count is named after the tier that writes it, as BatchMatcher.route_tiers():
// it is the length of the list the next tier reads (which list: engine.hip, RoutesStage / PathsStage).
enum CtlWord : int {
  kCtlPathUsed = 0,             // path pool used
  kCtlBallToSearch = 1,         // K2 ball tier -> search tiers
  kCtlErr = 2,                  // error flags (kErr*)
  kCtlLaneToReg2 = 3,           // routes: lane tier -> reg2
  kCtlPathsLaneToReg2 = 4,      // paths: the same
  kCtlReg2ToGroup = 5,          // routes: reg2 -> group tier
  kCtlPathsReg2ToGroup = 6,     // paths: the same
  kCtlK1LaneToWave = 7,         // K1 lane tier -> wave tier
  kCtlPathsBallToSearch = 8,    // path ball tier -> search tiers
  kCtlWaveToGlobal = 9,         // routes: 4096-slot wave tier -> global-memory tier
  kCtlPathsWaveToGlobal = 10,   // paths: the same
  kCtlGroupToWave512 = 11,      // routes: group tier -> 512-slot wave tier
  kCtlPathsGroupToWave512 = 12, // paths: the same
  kCtlWave512ToWave4096 = 13,   // routes: 512-slot tier -> 4096-slot tier
  kCtlPathsWave512ToWave4096 = 14,   // paths: the same
  kCtlWalkOverflow = 15,        // a K2 block's walk list overflowed (k_turn_walks_marked reads them all)
};
static_assert(kCtlWalkOverflow + 1 == kCtlWords, "one name per control word");
// Gate bits of DevBatch::gate: what a run without read-backs checks on the device instead (the host
// checks the same after the run and runs a gated-off batch again the ordinary way).
enum GateBit : uint32_t {
  // K4, the report and the segment gather skip a run whose path pool overflowed or whose records
  // exceed seg_cap (small_abort); set by every small and steady run
  kGateRecords = 1u,
  // ... and one that handed searches to the global-memory tier before its scratch exists
  kGateGlobal = 2u,
  // a steady run: every stage after the transition scan skips a batch with more transitions or K2
  // sources than trans_cap / src_cap, the pools an earlier run left (steady_abort)
  kGateSteady = 4u,
  // a steady run that did not launch the routes stage's hand-over tiers: items handed over after
  // all (kCtlBallToSearch) make K3 and everything after it skip
  kGateRoutesTiers = 8u,
  // likewise the path stage's tiers (kCtlPathsBallToSearch): K4 and the report skip
  kGatePathsTiers = 16u,
};
constexpr int kInlinePath = 8;  // path edges stored inline per slot (no allocation)

// Each group of buffers carries the capacity that sizes it, and is dropped as a whole by assigning
// it a fresh value (Workspace::drop); every buffer is a hipMalloc of its own.
struct WsPoints {   // sized by the batch's points, traces and option sets (Matcher::alloc_points)
  uint64_t cap_points = 0, cap_traces = 0, cap_opts = 0;
  // inputs
  DevBuf<uint32_t> trace_off; DevBuf<float> lon, lat; DevBuf<double> time;
  DevBuf<float> acc; DevBuf<MatchOptions> opts; DevBuf<uint32_t> trace_opt;
  // per slot
  DevBuf<uint32_t> slot_trace, n_states, state_orig;
  DevBuf<double> state_time;        // epoch time of the state at each slot (K4 interpolation)
  // candidate descriptors, 2 x uint4 per (slot, rank): {road, s_cm, len_cm, spf | spr << 16},
  // {node0, node1, time_ms(s_cm) forward from node0, time_ms(len_cm - s_cm) reverse from node1}
  // (sp* = mode-capped speed of the directed edge in 0.1 km/h, 0 when the mode cannot use it)
  DevBuf<uint8_t> cand_n; DevBuf<uint4> cand_desc; DevBuf<float> cand_sq;
  DevBuf<uint32_t> trans_cnt, trans_off; DevBuf<double> gc;
  DevBuf<uint4> pair_info;   // per layer pair slot: {route bound cm, time bound ms, KA | KB << 8 | mode << 16, 0}
  DevBuf<uint32_t> src_cnt, src_off;
  DevBuf<int8_t> choice; DevBuf<uint8_t> chain_start, bp;
  DevBuf<uint32_t> path_off, path_cnt, route_dist;
  DevBuf<uint2> path_sab;           // per chosen transition: source / target candidate offsets on their roads (cm)
  DevBuf<uint32_t> path_inline;     // kInlinePath edges per slot
  // per trace outputs
  DevBuf<uint32_t> seg_base, seg_cnt;
  DevBuf<uint32_t> trav_off;        // first traversal record of each slot (scan of path_cnt)
  DevBuf<uint32_t> rep_cnt; DevBuf<ReportStats> stats;
  DevBuf<uint32_t> ctl;   // the control words (CtlWord) and the hand-over lists they count
  DevBuf<uint32_t> rl_paths_a, rl_paths_b, rl_cand;
  DevBuf<uint32_t> rl_paths_c;      // global-memory search tier: the path stage's hand-over list (kCtlPathsWaveToGlobal)
  DevBuf<uint32_t> trace_err;               // per trace: error bits (kErr*) of that trace alone
  DevBuf<unsigned long long> tot64;         // u64 totals: [0] transitions [1] sources [2] path edges
  DevBuf<unsigned long long> scan_bkt;      // a steady run's coarse scan buckets (engine.hip BaseBuckets, rm_common.hpp scan_base_lane)
  DevBuf<unsigned long long> tot_part;      // per-block partial pairs of those totals (the scans fold them)
};
struct WsTrans {    // the transition pool
  uint64_t cap_trans = 0;
  DevBuf<uint32_t> route;
};
struct WsSrc {      // K2's sources and the routes stage's hand-over lists ((pair, source) items; c: kCtlWaveToGlobal)
  uint64_t cap_src = 0;
  DevBuf<uint32_t> src_item, rl_routes_a, rl_routes_b, rl_routes_0, rl_routes_c;
};
struct WsTurns {    // batches with turn costs only, allocated the first time one runs (Matcher::ensure_turns)
  uint64_t cap_turn = 0, cap_walk = 0;
  DevBuf<double> route_d;    // per transition: turn_m + |route_m - gc| (rule 3b)
  DevBuf<uint32_t> walk;     // K2 -> k_turn_walks: transitions whose turn weight is walked (item << 4 | target)
};
struct WsPath {     // the path pool
  uint64_t cap_path = 0;
  DevBuf<uint32_t> path_pool;
};
struct WsSegs {     // the record pools
  uint64_t cap_segs = 0;
  DevBuf<SegmentRec> segs;
  DevBuf<ReportRec> reps;
  DevBuf<uint32_t> rec_slot;   // K4: transition slot of each traversal record (k_rec_slot, or k_path_apply's fill)
};
// locality order (engine.hip k_loc_count / k_loc_scatter): the sorted state slots, each slot's
// region bucket, the bucket cursors and the item counts in sorted order; allocated on the first
// run that uses it (cap_sort slots)
struct WsSort {
  uint64_t cap_sort = 0;
  DevBuf<uint32_t> perm; DevBuf<uint16_t> loc_key; DevBuf<uint32_t> loc_cursor, pcnt;
};
struct Workspace : WsPoints, WsTrans, WsSrc, WsTurns, WsPath, WsSegs, WsSort {
  DevBuf<char> gsearch;   // global-memory search tier: its scratch, allocated on first use
  template <class Group>
  void drop() { static_cast<Group&>(*this) = Group{}; }
};

// Raw per-vehicle point stream (the trace files simple_reporter's download phase writes:
// uuid, time, lat, lon, accuracy per line, reference py/simple_reporter.py:113,139-140).
struct PointsDesc {
  uint64_t n_points = 0;
  const uint32_t* uuid = nullptr;      // dense vehicle index per point
  const double* time = nullptr;        // epoch seconds (integers in the reference)
  const float* lon = nullptr;
  const float* lat = nullptr;
  const float* accuracy = nullptr;     // < 0 when absent
  double inactivity = 120.0;           // --inactivity (simple_reporter.py:344)
  uint32_t n_uuids = 0;
  uint32_t n_opts = 0;
  const MatchOptions* opts = nullptr;
  const uint32_t* uuid_opt = nullptr;  // per vehicle index into opts (NULL: all use opts[0])
};

// Raw trace-file text for Matcher::parse_lines / run_lines (lines.hip): one chunk per file, lines
// in sv_lines.hpp's format; every window takes opts[0]
struct LinesDesc {
  uint32_t n_chunks = 0;
  const char* const* data = nullptr;
  const uint64_t* len = nullptr;
  sv::Format fmt;
  double inactivity = 120.0;
  uint32_t n_opts = 0;
  const MatchOptions* opts = nullptr;
};
struct LineState;   // lines.hip: the device buffers and the last call's results of the line reader
// the generic rule over the same input on the host alone (no GPU); null arrays are not written,
// info as Matcher::lines_info
void lines_parse_host(const LinesDesc& d, uint64_t info[7], uint32_t* uuid, double* time, float* lon, float* lat, float* acc,
                      uint32_t* v_chunk, uint64_t* v_off, uint32_t* v_len);
// The process's date patterns (DESIGN.md §3 rule 18; lines.hip).  register: the pattern compiled
// and kept -> the id (16 and up) to put into sv::Format::time_format, the same id for the same
// text, or -1 with the reason in err.  find: null for an id nobody registered.  Both thread-safe;
// a found pattern stays where it is for the life of the process.
int32_t time_pattern_register(const char* pattern, std::string& err);
const tp::Pattern* time_pattern_find(int32_t id);

// Raw stream messages for Matcher::parse_messages (lines.hip; DESIGN.md §3 rule 14): chunks as in
// LinesDesc, one message per line, either kind of msg::Format
struct MessagesDesc {
  uint32_t n_chunks = 0;
  const char* const* data = nullptr;
  const uint64_t* len = nullptr;
  msg::Format fmt;
  int strict = 0;          // 1: the first malformed line fails the call; 0: it is dropped and counted
  int has_stamp = 0;       // 1: every message carries stamp_ms; 0: (int64)(time * 1000) of its own
  int64_t stamp_ms = 0;
};
struct DroppedMessage {
  uint32_t chunk;          // both 1-based
  uint64_t line;
  const char* why;
};
// what the line reader left on the device for the directory and the session: the kept points in
// input order, numbered per call in first-seen order, and each number's name span in the text
struct LineGroups {
  uint64_t n_points = 0;
  uint32_t n_groups = 0;
  const uint8_t* text = nullptr;
  const uint32_t* v_off = nullptr;
  const uint32_t* v_len = nullptr;
  uint32_t* p_uuid = nullptr;
  const double* p_time = nullptr;
  const float* p_lon = nullptr;
  const float* p_lat = nullptr;
  const float* p_acc = nullptr;
  unsigned long long hash_mask = ~0ull;   // RM_LINES_HASH_BITS
};
// the generic rule over the same input on the host alone (no GPU); null arrays are not written;
// info: Matcher::lines_info's seven and the dropped messages
void messages_parse_host(const MessagesDesc& d, uint64_t info[8], uint32_t* uuid, double* time, float* lon, float* lat, float* acc,
                         uint32_t* v_chunk, uint64_t* v_off, uint32_t* v_len, std::vector<DroppedMessage>* dropped);

// Time-tile stage parameters (simple_reporter.py:176-196, 211-254; CLI defaults :343,345,346)
struct TileParams {
  uint32_t quantisation = 3600;
  uint32_t privacy = 2;
  std::string source = "smpl_rprt";
  std::string mode = "AUTO";
};

// one CSV row of a time tile (simple_reporter.py:192-195) plus its sort keys
struct TileRow {
  uint64_t id, next_id;
  int64_t start, end;                  // floor(t0), ceil(t1)
  int32_t duration, length, queue;
  uint32_t bucket;                     // floor(time / quantisation)
  uint32_t tile;                       // level | tile index << 3 (id & 0x1FFFFFF)
  uint32_t pad[3];
};
static_assert(sizeof(TileRow) == 64, "TileRow is four dwordx4");

struct StageBufs {  // grow-only device buffers of the windowing and tile stages
  uint64_t cap_pts = 0, cap_rows = 0;
  uint32_t cap_tr = 0, cap_uuids = 0;
  DevBuf<uint32_t> derr, p_uuid, p_uopt;
  DevBuf<double> p_time;
  DevBuf<float> p_lon, p_lat, p_acc;
  DevBuf<MatchOptions> p_opts;
  DevBuf<unsigned long long> k0, k1, rk, rk2;
  DevBuf<uint32_t> v0, v1, flag, idx, wstart, wcnt, wofs, wflag, widx, trace_uuid;
  DevBuf<TileRow> rows, rows2;
  DevBuf<uint32_t> rperm, rperm2, rflag, ridx, gpos, tcnt, tofs;
  DevBuf<uint8_t> gkeep;
  ScanScratch scr;                     // sized with the buffers (ensure_points, ensure_rows)
  PinBuf<uint32_t> hctl;               // pinned read-back words
};

// error bits in ctl[kCtlErr] (and, except the path pool, per trace in Workspace::trace_err)
constexpr uint32_t kErrCandOverflow = 1u, kErrSearchOverflow = 2u, kErrPathOverflow = 4u, kErrRounds = 8u;
// message of the first error bit set in `bits` ("" for none)
const char* error_text(uint32_t bits);

class Engine;
class Matcher;

// Vehicle sessions (DESIGN.md §3 rule 12; sessions.hip): the streaming batcher of the reference
// (BatchingProcessor.java, Batch.java) kept in HBM beside a matcher.  Same layouts as
// rm_session_params' scalar part, rm_session_report and rm_session_window (reporter_match.h).
struct SessionParams {
  double report_dist_m = 500.0;     // BatchingProcessor.java:28
  uint32_t report_count = 10;       // :27
  double report_time_s = 60.0;      // :26
  int64_t session_gap_ms = 60000;   // :29
  uint32_t max_vehicle_points = 0;  // 0: unbounded (the reference)
  MatchOptions opt = default_options();
  RunParams run;
};
struct SessionPoints {
  uint64_t n = 0;
  const uint32_t* vehicle = nullptr;
  const double* time = nullptr;
  const float* lon = nullptr;
  const float* lat = nullptr;
  const float* accuracy = nullptr;     // may be null: -1, absent
  const int64_t* stamp_ms = nullptr;   // stream time of each arrival
};
struct SessionReport {
  ReportRec r;
  uint32_t vehicle, window;   // window: index into the call's window records
};
static_assert(sizeof(SessionReport) == 56, "SessionReport is rm_session_report");
constexpr uint32_t kSessCapped = 0x80000000u;   // SessionWindow::err: cleared at max_vehicle_points, not matched
struct SessionWindow {
  uint32_t vehicle, arrival, n_points;   // arrival: index in the push of the triggering point (punctuate: the vehicle)
  int32_t shape_used;                    // -1 when absent
  uint32_t n_reports, err;               // reports before the forwarding filter; the trace's error bits
};
static_assert(sizeof(SessionWindow) == 24, "SessionWindow is rm_session_window");

// what snapshot.hip sees of a session (DESIGN.md §3 rule 15): the per-vehicle state and the current
// point buffer, on `stream`
struct SessionSnap {
  uint32_t n_vehicles = 0, n_live = 0;   // n_live: vehicles holding points (after snapshot_pack)
  uint64_t n_points = 0;
  uint32_t* off = nullptr; uint32_t* cnt = nullptr; uint32_t* scan_from = nullptr; uint32_t* try_from = nullptr;
  float* max_sep = nullptr; long long* last_update = nullptr;
  uint32_t* rank = nullptr;   // n_vehicles + 1 words: after snapshot_pack each vehicle's rank among the non-empty ones
  float* lon = nullptr; float* lat = nullptr; float* acc = nullptr; double* time = nullptr;
  uint32_t* arr = nullptr; uint32_t* veh = nullptr;
  hipStream_t stream = nullptr;
};

class Session {
 public:
  Session(Matcher* m, uint32_t n_vehicles, const SessionParams& sp);
  ~Session();
  Session(const Session&) = delete;
  Session& operator=(const Session&) = delete;
  // out: arrivals evaluated, triggers, trims, cleared by an absent shape_used, failed windows,
  // forwarded reports, invalid reports, rounds
  void push(const SessionPoints& pts, uint64_t out[8]);
  // push() from where its staging ends: n arrivals already in HBM on the session's GPU (d_acc may
  // be null).  d_stamp null: every arrival carries `stamp` when has_stamp, else (int64)(time * 1000)
  // of its own.  The arrays are read before the first match round and may lie in the runner's
  // stage buffers.
  void push_device(uint64_t n, const uint32_t* d_vehicle, const double* d_time, const float* d_lon, const float* d_lat,
                   const float* d_acc, const long long* d_stamp, bool has_stamp, int64_t stamp, uint64_t out[8]);
  // The masked push of a sharded stream (DESIGN.md §3 rule 16): of the n arrivals only those whose
  // vehicle_owner(vehicle, nranks) is `rank` are appended, triggered and matched; a window's arrival
  // stays the index among all n.  shard: the own points, the foreign points
  void push_device_sharded(uint64_t n, const uint32_t* d_vehicle, const double* d_time, const float* d_lon, const float* d_lat,
                           const float* d_acc, const long long* d_stamp, bool has_stamp, int64_t stamp, int nranks, int rank,
                           uint64_t out[8], uint64_t shard[2]);
  void punctuate(int64_t timestamp_ms, uint64_t out[8]);
  // throws what a push of n arrivals would throw for lack of room, before anything is changed
  void check_room(uint64_t n) const;
  uint64_t n_reports() const;   // of the last call
  uint64_t n_windows() const;
  void get_reports(SessionReport* out);
  void get_windows(SessionWindow* out);
  // the store packed by vehicle: cnt, max_sep, last_update (n_vehicles each) and the kept points
  // (sum of cnt; null arrays are not written); returns the point count
  uint64_t get_store(uint32_t* cnt, float* max_sep, int64_t* last_update, float* lon, float* lat, double* time, float* acc);
  void times(double ms[5]) const;   // upload, append, trigger, match, trim of the last call
  uint32_t n_vehicles() const;
  // for a TileStore fed device-to-device: the session's GPU and the last call's forwarded
  // reports in HBM (n_reports() of them, complete when the call has returned)
  int device() const;
  const SessionReport* reports_device() const;
  // ... the last call's windows in HBM (n_windows(), ordered as get_windows gives them), and whether
  // a sharded push was ever made: the tile store then keys the rows it takes from here (rule 16)
  const SessionWindow* windows_device() const;
  bool sharded() const;
  // the stream snapshot (rule 15).  snapshot_pack: the store packed as get_store packs it (no
  // output of the stream changes), the non-empty vehicles ranked.  snapshot_room: the current
  // buffer with room for n points, for a session that holds none.  snapshot_loaded: n points and
  // their vehicles' state are in place; the last call's windows and reports are empty.
  hipStream_t stream() const;   // the runner's
  SessionSnap snapshot_pack();
  SessionSnap snapshot_room(uint64_t n_points);
  void snapshot_loaded(uint64_t n_points);
  void snapshot_clear();   // every vehicle empty, as created (a load that failed half way)
  void snapshot_sharded();   // a load of shards (rule 17): the next add_session from here keeps keys

 private:
  struct Impl;
  std::unique_ptr<Impl> p_;
  SessionSnap snap_view(uint64_t n_points, uint32_t n_live);
  void match_round(uint32_t T, uint64_t P, bool evict);
  void rounds(bool evict, uint64_t out[8]);
  void finish_call(uint64_t out[8]);
  void append(uint64_t n, const uint32_t* d_veh, const double* d_time, const float* d_lon, const float* d_lat, const float* d_acc,
              const long long* d_stamp, uint64_t out[8]);
};

// The vehicle directory (DESIGN.md §3 rule 14; directory.hip): the map from id bytes to a dense
// index that lasts across calls, kept in HBM as an open-addressed table and an arena of names.
class Directory {
 public:
  Directory(int device, uint32_t max_vehicles);
  ~Directory();
  Directory(const Directory&) = delete;
  Directory& operator=(const Directory&) = delete;
  // Give every kept point of the matcher's last parse its directory index (in g.p_uuid, which
  // holds the per-call number on entry), new ids numbered in first-seen order behind the known
  // ones.  Throws "directory full", before anything is written, when they would pass max_vehicles.
  void assign(Matcher& m);
  uint32_t size() const;
  uint32_t max_vehicles() const;
  int device() const;
  // vehicles [first, first + n): off (n + 1 entries, from 0) into `bytes`; null arrays are not
  // written; returns the bytes of the range
  uint64_t names(uint32_t first, uint32_t n, uint64_t* off, char* bytes);
  double last_ms() const;   // device time of the last assign
  // the stream snapshot (rule 15).  snapshot_gather: the names' offsets (size() + 1) and bytes
  // (name_bytes()) in index order into device memory.  snapshot_insert, into an empty directory:
  // name k of the n at d_off / d_bytes gets index k under this process's hash mask; two equal
  // names set bit dup_bit of *d_err.  snapshot_clear: empty again, as created.
  uint64_t name_bytes() const;
  void snapshot_gather(unsigned long long* d_off, uint8_t* d_bytes, hipStream_t st);
  void snapshot_insert(uint32_t n, const unsigned long long* d_off, const uint8_t* d_bytes, uint64_t n_bytes,
                       unsigned long long* d_err, uint32_t dup_bit, hipStream_t st);
  void snapshot_clear(hipStream_t st);

 private:
  struct Impl;
  std::unique_ptr<Impl> p_;
};

// The tile store (DESIGN.md §3 rule 13; tilestore.hip): the reference's streaming anonymiser
// (AnonymisingProcessor.java, TimeQuantisedTile.java, Segment.java:38-74) kept and flushed in HBM.
// TileSegment has the layout of rm_tile_segment (reporter_match.h) and of ReportRec's first 40 bytes.
struct TileSegment {
  uint64_t id, next_id;
  double t0, t1;
  int32_t length, queue_length;
};
static_assert(sizeof(TileSegment) == 40, "TileSegment is rm_tile_segment");
class TileStore {
 public:
  // tp.mode as printed (upper-cased by the caller); initial_rows: the first capacity (it doubles)
  TileStore(int device, const TileParams& tp, uint64_t initial_rows);
  ~TileStore();
  TileStore(const TileStore&) = delete;
  TileStore& operator=(const TileStore&) = delete;
  // out: segments kept, segments skipped as !valid(), rows appended, rows held.  A segment
  // outside rule 13's stated limits fails the call and leaves the store as it was.
  void add(const TileSegment* segs, uint64_t n, uint64_t out[4]);
  void add_session(Session& s, uint64_t out[4]);   // the session's last push / punctuate
  // punctuate: *blob is malloc'd ("name\0body\0" per file, files by (start, tile id)); out: rows
  // in, rows kept, tiles held, files written, blob bytes.  The store is empty afterwards.
  void flush(char** blob, size_t* len, uint64_t out[5]);
  void times(double ms[6]) const;   // upload, expand, sort, cull, text, download of the last call
  // The sharded stream's exchange (DESIGN.md §3 rule 16).  Every row has a key beside it, add call
  // << 32 | a (a session's report: its triggering arrival; host segments: the index in the array),
  // kept from the first of these calls or the first add_session of a sharded session on; a store
  // that sees neither allocates and launches nothing for keys.
  // export_rows: *blob is malloc'd, the rows held and their keys; the store keeps them.
  // import_owned: the store's contents are replaced by the rows of the n blobs (in rank order)
  // whose file tile_file_owner gives to `rank`, merged by one stable sort on the key.
  // exchange: the same with the rows all-gathered on the device through `comm`.
  // out: rows before, rows sent away, rows received, rows held.
  void export_rows(char** blob, size_t* len);
  void import_owned(const char* const* blobs, const size_t* lens, uint32_t n, int nranks, int rank, uint64_t out[4]);
  void exchange(struct TileComm& comm, uint64_t out[4]);
  void exchange_times(double ms[3]) const;   // partition, transport, merge of the last import / exchange
  bool keyed() const;
  int device() const;
  uint64_t rows_held() const;
  uint64_t capacity() const;
  // the stream snapshot (rule 15): the rows held in store order, the running arrival number, and
  // a load's two steps: room for n rows in an empty store (grown as add grows it), then n rows in place
  const void* rows_device() const;
  uint64_t arrivals() const;
  uint32_t quantisation() const;
  hipStream_t stream() const;
  void* snapshot_room(uint64_t n_rows);
  void snapshot_loaded(uint64_t n_rows, uint64_t arrivals);
  // a sharded stream's snapshot (rule 17).  snapshot_keys: the store keeps keys from here on (the
  // rows held get theirs) and the keys held, in store order.  calls: the add calls numbered so far.
  // snapshot_merge, into an empty store: of the n_parts ranges of rows (device memory, in rank order;
  // keys[i] null: that range's rows are keyed by their position under call 0) those whose file
  // `rank` owns, through the exchange's own merge; the store is keyed afterwards and carries on at
  // `calls` and `arrivals`.  A throw leaves the store empty.  snapshot_clear: empty again.
  const void* snapshot_keys();
  uint64_t calls() const;
  void snapshot_merge(const void* const* rows, const void* const* keys, const uint64_t* counts, uint32_t n_parts, int nranks,
                      int rank, uint64_t calls, uint64_t arrivals);
  void snapshot_clear();

 private:
  struct Impl;
  std::unique_ptr<Impl> p_;
};

// The stream snapshot (DESIGN.md §3 rule 15; snapshot.hpp, snapshot.hip).  Any object may be null.
// save: *blob is malloc'd; out: bytes, names, vehicles, points, rows, user bytes; ms: pack, gather,
// checksum, download.  load, into empty objects: out: bytes, names, vehicles, points, rows, user
// bytes; ms: upload, check, unpack.  A load that throws leaves its targets empty and usable.
void snapshot_save(Session* s, Directory* d, TileStore* t, const char* user, size_t user_len, char** blob, size_t* len,
                   uint64_t out[6], double ms[6]);
void snapshot_load(Session* s, Directory* d, TileStore* t, const char* blob, size_t len, uint64_t out[6], double ms[6]);
// The snapshot of a stream on several ranks (DESIGN.md §3 rule 17).  save_shard: rank's blob of
// nranks -- its sessions, the directory, its rows, their keys and the shard record (the store is
// needed); out and ms as for save.  load_shards, into empty objects: of the n blobs of one save
// (any order; one blob without a shard record counts as rank 0 of 1) what `rank` of `nranks` holds.
// out: bytes of all blobs, names, vehicles held, points held, rows held, user bytes of the first
// blob, calls, saved ranks; ms: upload, check, unpack, rows (the store's merge)
void snapshot_save_shard(Session* s, Directory* d, TileStore* t, int rank, int nranks, const char* user, size_t user_len,
                         char** blob, size_t* len, uint64_t out[6], double ms[6]);
void snapshot_load_shards(Session* s, Directory* d, TileStore* t, const char* const* blobs, const size_t* lens, uint32_t n,
                          int rank, int nranks, uint64_t out[8], double ms[6]);
unsigned long long lines_hash_mask();   // RM_LINES_HASH_BITS as the line reader reads it (lines.hip)

// report() (reference py/reporter_service.py:79-179) on the device over host-supplied segment
// lists: trace k's segments are segs[seg_off[k] .. seg_off[k+1]); reports come back compacted
// (rep_off, T+1) with per-trace stats.  reps must hold seg_off[T] records.
void report_segments(int device, uint32_t T, const uint32_t* seg_off, const SegmentRec* segs, const double* end_time,
                     const double* threshold, const uint32_t* rmask, const uint32_t* tmask, uint32_t* rep_off,
                     ReportRec* reps, ReportStats* stats);
// the same, left in HBM (T >= 1): trace k's reports are reps[seg_off[k] .. + stats[k].n_reports)
struct DeviceReports {
  DevBuf<uint32_t> seg_off, seg_cnt;
  DevBuf<SegmentRec> segs;
  DevBuf<ReportRec> reps;
  DevBuf<ReportStats> stats;
};
void report_segments_device(int device, uint32_t T, const uint32_t* seg_off, const SegmentRec* segs, const double* end_time,
                            const double* threshold, const uint32_t* rmask, const uint32_t* tmask, DeviceReports& out);

// ---- the /report reply (DESIGN.md §3 rule 19; reply.hip, reply_text.hpp) ----
// Both writers give the n replies in one malloc'd, NUL-terminated buffer: reply i is
// (*buf)[off[i], off[i+1]) (off: T + 1 entries).  A trace holding a time outside the time routine's
// range is flagged and written with std::to_chars by either writer (the device writer splices it in
// on the host after the download); *flagged counts them.
// host: trace k's segments are segs[seg_off[k] .. seg_off[k+1]), its reports reps[rep_base[k] .. + rep_cnt[k])
void reply_format_host(uint32_t T, const uint32_t* seg_off, const SegmentRec* segs, const uint32_t* rep_base,
                       const uint32_t* rep_cnt, const ReportRec* reps, const ReportStats* stats, char** buf, uint64_t* off,
                       uint64_t* flagged);
// one trace's reply into a string (a coalesced request's caller formats its own)
void reply_format_one(const SegmentRec* segs, uint32_t S, const ReportRec* reps, uint32_t R, const ReportStats& st, std::string& o);
// device: the records of T traces in HBM; trace k's segments are segs[seg_base[k] .. + seg_cnt[k]), its
// reports reps[rep_base[k] .. + stats[k].n_reports); cap: the records either pool holds
struct ReplySource {
  uint32_t T = 0;
  const uint32_t* seg_base = nullptr;
  const uint32_t* seg_cnt = nullptr;
  const uint32_t* rep_base = nullptr;
  const SegmentRec* segs = nullptr;
  const ReportRec* reps = nullptr;
  const ReportStats* stats = nullptr;
  uint64_t cap = 0;
};
// The device writer with its grow-only buffers.  write() runs on st and returns synchronised;
// *ms: its kernels' and scans' device time.
class ReplyWriter {
 public:
  void write(int device, hipStream_t st, const ReplySource& src, char** buf, uint64_t* off, uint64_t* flagged, double* ms);

 private:
  DevBuf<uint32_t> flag_, item_trace_;
  DevBuf<unsigned long long> cnt_, ioff_, roff_, len_, ofs_;
  DevBuf<char> blob_;
  PinBuf<unsigned long long> hn_;
  uint64_t t_cap_ = 0, i_cap_ = 0, blob_cap_ = 0;
  ScanScratch scr_{"reply buffers do not fit in HBM"};
  PartTimer timer_;
};
// runs at or below this many points are written on the host (RM_REPLY_DEVICE_MIN_POINTS, read per
// call; default: the matcher's small-run limit)
uint64_t reply_device_min_points();

// The tile stage's collectives (one process per GPU): RCCL over xGMI, or a host transport the
// caller injects (capi.cpp rm_comm_init_host).  Both are blocking on `st`.
struct TileComm {
  int rank = 0, nranks = 1;
  virtual ~TileComm() = default;
  virtual uint64_t max_u64(uint64_t v, hipStream_t st) = 0;
  // every rank's `bytes` device bytes at send, in rank order, into recv (nranks * bytes)
  virtual void allgather(const void* send, void* recv, size_t bytes, hipStream_t st) = 0;
};

class Matcher {
 public:
  explicit Matcher(Engine* e);
  ~Matcher();
  Matcher(const Matcher&) = delete;
  Matcher& operator=(const Matcher&) = delete;
  friend class Session;

  // Upload a batch and run every stage on this matcher's stream; returns when the run's control
  // words are back (a large batch also reads its transition and path totals back between the
  // stages; a small one sizes its pools from upper bounds instead: run_small).  Throws on error.
  void run(const HostBatch& b, const RunParams& rp);
  // Run every stage over the batch already resident in HBM (inputs of the last run()).
  void run_device(const RunParams& rp);
  // rm_match_batch's device JSON path (engine.hip k_parse_json): reserve the byte buffer, upload
  // the trace-array bytes (from the parse threads, as their arenas fill), reserve the workspace,
  // parse them into the point arrays (flags[k] != 0:
  // trace k was not in the compact layout and must be parsed on the host; tspan[2k], [2k+1]: its
  // first and last times), place host-parsed traces' points, then run with the points in place
  void json_reserve_bytes(uint64_t bytes);                               // the byte buffer
  void json_reserve(uint64_t points, uint32_t traces, uint32_t nopts);     // workspace + per-trace arrays
  void json_upload(uint64_t off, const void* src, uint64_t n);             // thread-safe
  // span[2k], span[2k+1]: trace k's bytes [begin, end) in the buffer (begin == end: host-parsed)
  void json_parse(const uint64_t* span, const uint32_t* trace_off, uint32_t T, uint32_t* flags, double* tspan);
  void upload_points(uint64_t first, uint64_t n, const float* lon, const float* lat, const double* time, const float* acc);
  void run_parsed(const uint32_t* trace_off, uint32_t T, const MatchOptions* opts, uint32_t n_opts,
                  const uint32_t* trace_opt, const double* tspan, const RunParams& rp);
  void sync();
  // sizes of the last run
  uint32_t n_traces() const { return n_traces_; }
  uint64_t n_points() const { return n_points_; }
  uint64_t n_trans() const { return n_trans_; }
  uint64_t n_path_edges() const { return n_path_; }
  uint64_t seg_pool_used() const { return seg_used_; }
  // downloads of the last run (host buffers sized by the caller)
  void get_states(uint32_t* n_states, uint32_t* state_orig);
  void get_candidates(uint8_t* cand_n, uint32_t* road, uint32_t* s_cm, float* sq);
  void get_routes(uint32_t* trans_off, double* gc, uint32_t* route);
  // the distance terms K3 used (n_trans() doubles); 0 (nothing written) when the batch had no turn costs
  int get_route_terms(double* route_d);
  void get_viterbi(int8_t* choice, uint8_t* chain_start);
  void get_paths(uint32_t* path_off, uint32_t* path_cnt, uint32_t* pool, uint32_t* route_dist);
  // segments compacted per trace: seg_off (T+1), segs (seg_off[T])
  void get_segments(uint32_t* seg_off, SegmentRec* segs);
  // the same with the buffers sized from the device counts (one count read-back, not two)
  void get_segments(std::vector<uint32_t>& seg_off, std::vector<SegmentRec>& segs);
  uint64_t count_segments();
  void get_reports(uint32_t* rep_off, ReportRec* reps, ReportStats* stats);
  uint64_t count_reports();
  // a Report run's records for the host writer, and where they lie in HBM for the device writer
  void get_report_records(std::vector<uint32_t>& seg_off, std::vector<SegmentRec>& segs, std::vector<uint32_t>& rep_base,
                          std::vector<uint32_t>& rep_cnt, std::vector<ReportRec>& reps, std::vector<ReportStats>& stats);
  struct ReplySource reply_source();
  // Matched points of the last run()/rerun (rule 9; points.hip): one record per input point in
  // batch point order (n_points()), computed on request from what the run left in HBM
  void matched_points(MatchedPoint* out);
  // Matched edges of the last run()/rerun (rule 10; edges.hip): every edge visit of every chain
  // with its times, and each trace's matched polyline, computed on request from what the run left
  // in HBM and kept on the device.  out: visits, shape vertices (of the whole batch)
  void matched_edges(uint64_t out[2]);
  // the result of the last matched_edges(): edge_off / shape_off (n_traces + 1 each; trace k's
  // visits and vertices), the visits, the vertices as (lon, lat) pairs
  void get_matched_edges(uint32_t* edge_off, MatchedEdge* edges, uint32_t* shape_off, float* shape);
  // device time (ms) of the last matched_edges(): HIP events round its launches
  double matched_edges_ms() const { return me_ms_; }
  // accumulated kernel time (ms) per KernelId since the last reset
  void kernel_times(double* ms, uint64_t* launches);
  // overflow-list sizes of the last run: routes A, routes B, paths A, candidates
  void tier_counts(uint32_t* out4);
  // the kCtlWords control words of the last run (zeros before any run)
  void ctl_words(uint32_t* out);
  // since creation: [0] steady runs [1] steady runs gated off and run again the ordinary way
  // [2] steady runs without the routes stage's hand-over tiers [3] ... without the path stage's
  void run_stats(uint64_t* out4) const;
  void reset_kernel_times();
  void set_timing(bool on) { timing_mask_ = on ? ~0u : 0u; }
  void set_timing_mask(uint32_t mask) { timing_mask_ = mask; }   // bit k: stage k (kernel_name)
  // Failure isolation: off (default), a trace that fails (kErrCandOverflow / kErrSearchOverflow /
  // kErrRounds) makes run() throw; on, run() returns, the failed traces carry no segments or
  // reports and their bits are in get_trace_errors().  The reference fails one request
  // (py/reporter_service.py:244-245) or skips one window (py/simple_reporter.py:169-173).
  void set_isolation(bool on) { isolate_ = on; }
  // Locality order of the stages that read the graph's regional data: 0 slot order, 1 K1 and K2
  // sorted by region, 2 the path stage too, -1 auto (2 on graphs of Engine::locality_default, 1
  // for batches sampled every >= 10 s on smaller ones, else 0).  Results are identical in every
  // mode.  Env RM_LOCALITY sets the initial value.
  void set_locality(int mode) { locality_ = mode; }
  bool locality_used() const { return locality_used_; }
  uint32_t error_bits() const { return err_bits_; }   // OR of the last run's per-trace errors
  void get_trace_errors(uint32_t* out);                // n_traces() words
  hipStream_t stream() const { return stream_; }
  const Engine& engine() const { return *eng_; }

  // Raw point stream -> per-vehicle time sort and inactivity windows of >= 2 points on the
  // GPU (simple_reporter.py:137-164), then every matching stage over the windows.
  void run_points(const PointsDesc& pd, const RunParams& rp);
  // The same from the points already in StageBufs (p_uuid, p_time, p_lon, p_lat, p_acc): everything
  // from k_pt_keys on.  n_uopt: vehicles with an option index in p_uopt (0: all take opts[0]);
  // windows_done: its open part is closed once the windows are built, before the matcher runs
  void run_points_device(uint64_t n, double tbase, double inactivity, const MatchOptions* opts, uint32_t n_opts,
                         uint32_t n_uopt, const RunParams& rp, PartTimer* windows_done = nullptr);
  // Trace-file text -> points on the device (lines.hip; DESIGN.md §3 rule 11): lines parsed by
  // k_line_parse (the generic host reader for lines outside the compact layout), the kept points
  // packed in input order into StageBufs, vehicle ids numbered in first-seen order.  run_lines
  // then windows and matches them as run_points does.  Throws "chunk <c> line <l>: <reason>".
  void parse_lines(const LinesDesc& d);
  void run_lines(const LinesDesc& d, const RunParams& rp);
  // Stream messages -> points on the device (DESIGN.md §3 rule 14): parse_lines with either kind
  // of message and, when !d.strict, malformed lines dropped and counted instead of thrown
  void parse_messages(const MessagesDesc& d);
  uint64_t dropped_messages(std::vector<DroppedMessage>* first) const;   // of the last parse (first: at most 64)
  LineGroups line_groups() const;                                          // of the last parse
  bool line_time_span(double t[2]) const;   // smallest and largest time of its kept points (false: none)
  int device() const;
  // lines, blank, outside the box, points, vehicles, lines read on the host, 1: ids assigned on the host
  void lines_info(uint64_t out[7]) const;
  void get_line_points(uint32_t* uuid, double* time, float* lon, float* lat, float* acc);   // input order
  void get_vehicles(uint32_t* chunk, uint64_t* off, uint32_t* len);   // name span per vehicle
  void lines_time(double ms[4]) const;   // upload, parse (+ host lines), ids, windows
  // Gzip chunks (inflate.hip; DESIGN.md §3 rule 20): how parse_lines, run_lines and parse_messages
  // read their chunks from now on.  0 plain (the default), 1 gzip, 2 gzip where a chunk begins
  // 1f 8b.  A bad chunk throws "chunk <c>: gzip: <reason>" (the first in input order), or with
  // skip_bad counts as empty.  The inflated text lives on the device only: get_text reads it back.
  void set_input_coding(int coding, bool skip_bad);
  uint32_t chunk_count() const;                // chunks of the last parse
  void chunk_status(uint32_t* status) const;   // rule 20's status of every chunk of the last parse (0 for plain ones)
  // chunks inflated, members, bytes in, bytes out, second-pass chunks, chunks inflated on the host
  void inflate_info(uint64_t out[6]) const;
  void inflate_time(double ms[3]) const;       // inflate (with the CRC), 0, gather
  void get_text(uint32_t chunk, uint64_t off, uint64_t len, char* out);   // bytes of the last parse's text
  // vehicle index of every window of the last run_points (n_traces entries)
  void get_trace_uuid(uint32_t* out);
  // the batch the last run matched (after run_points: the windows built on the device)
  void get_batch(uint32_t* trace_off, float* lon, float* lat, double* time, float* acc);
  // Time tiles of the last run's reports: hour buckets, sort, privacy cull of (id, next_id)
  // runs and CSV text (simple_reporter.py:176-254).  Returns "name\0body\0" per file.  With
  // a communicator, rows of every rank are all-gathered and each rank emits the files it owns.
  std::string tiles(const TileParams& tp, struct TileComm* comm = nullptr);

 private:
  void parse_text(const MessagesDesc& d, const tp::Pattern* pat);
  void ensure(uint64_t points, uint32_t traces, uint32_t nopts);
  void check_batch(uint32_t T, const uint32_t* trace_off, const MatchOptions* opts, uint32_t n_opts,
                   const uint32_t* trace_opt);
  void scan_options(const MatchOptions* opts, uint32_t n_opts);
  // device JSON path (grow-only): the trace-array bytes (jcap_ of them and a kJsonPad tail), and
  // per trace (jtcap_) its span, flag and first / last times
  DevBuf<char> jdev_;
  uint64_t jcap_ = 0;
  DevBuf<uint64_t> jspan_;
  DevBuf<uint32_t> jflag_;
  DevBuf<double2> jtsp_;
  uint32_t jtcap_ = 0;
  void ensure_trans(uint64_t n, uint64_t n_src);
  void ensure_path(uint64_t n);
  void ensure_segs(uint64_t n);
  void ensure_turns();
  // the same, throwing OutOfDeviceMemory (ensure() retries a failed grown size at the exact one)
  void alloc_points(uint64_t cp, uint64_t ct, uint64_t co, uint64_t keep_trans, uint64_t keep_path, uint64_t keep_segs,
                    uint64_t keep_src);
  void ensure_trans_raw(uint64_t n, uint64_t n_src);
  void ensure_path_raw(uint64_t n);
  void ensure_segs_raw(uint64_t n);
  void ensure_global_search();
  void read_ctl();
  void tic(int k) { if ((timing_mask_ >> k) & 1u) timer_.tic(k, stream_); }
  void toc(int k) { if ((timing_mask_ >> k) & 1u) timer_.toc(stream_); }
  // per-trace record lists (base[k], cnt[k] in units of `words` u64) compacted on the device and
  // downloaded through pinned memory into dst; off gets the T+1 offsets
  void download_compacted(const uint32_t* d_base, const uint32_t* d_cnt, const void* d_src, uint32_t words,
                          uint32_t* off, void* dst, const std::function<void*(uint64_t)>& dst_for);
  void grow_dl_host(size_t need);
  bool download_prefetched(uint32_t* off, void* dst, const std::function<void*(uint64_t)>& dst_for);
  void grow_dl_dev(size_t need);
  // small batches (run_small): no size read-back between the stages, one upload, one read-back
  bool run_small(const RunParams& rp, const DevGraph& g);
  // large batches once a run has sized the pools: no read-back between the stages (run_steady)
  bool run_steady(const RunParams& rp, const DevGraph& g);
  // the stage launches the three run paths share, written once (engine.hip: they take the kernels'
  // view of the batch, a type of that file); what differs between the paths is a LaunchPlan
  struct Stages;
  void read_back(bool totals);
  void finish_run(const RunParams& rp);
  bool route_balls(const DevGraph& g) const;   // some mode of the batch has route balls
  // the pinned mirror of Workspace::tot64, behind the control words
  unsigned long long* htot() const { return reinterpret_cast<unsigned long long*>(hctl_ + kCtlWords); }
  uint64_t steady_src_ = 0;    // the last ordinary / steady run's K2 sources (0: no steady run yet)
  uint32_t steady_ctl_[kCtlWords] = {0};   // ... and its control words (the hand-over lists' lengths)
  uint32_t clean_routes_ = 0, clean_paths_ = 0;   // completed runs in a row (at most 2) with a stage's lists empty
  uint64_t run_stats_[4] = {0, 0, 0, 0};          // run_stats()
  void keep_ctl();
  void count_clean(const uint32_t* ctl);
  void zero_hist(const RunParams& rp);
  void use_ws_inputs();
  void ensure_pack(uint64_t bytes);

  Engine* eng_;
  // Every member below frees itself after ~Matcher's body, which synchronises and destroys the
  // stream first: none of them needs the stream to go.
  hipStream_t stream_ = nullptr;
  InputView in_;
  PinBuf<char> hpack_;         // pinned staging and device block of a small run()'s inputs (grow-only,
  DevBuf<char> dpack_;         // both of dpack_.cap() bytes)
  PinBuf<uint32_t> hoff_;      // pinned: a small run's per-trace segment offsets (T + 1), prefetched
  DevBuf<uint32_t> levels_dev_;    // a Report run's per-trace level masks (report, then transition) and
  PinBuf<uint32_t> levels_host_;   // their pinned staging (grow-only, both of levels_dev_.cap() words)
  bool levels_on_ = false;         // the current run reads them
  bool seg_prefetched_ = false;
  bool rep_prefetched_ = false;    // ... and its reports beside them, rep_prefetch_at_ bytes into dl_dev_
  size_t rep_prefetch_at_ = 0;
  DevBuf<char> dl_dev_;        // grow-only device / pinned host buffers of download_compacted
  PinBuf<char> dl_host_;
  DevBuf<MatchedPoint> mp_dev_;   // grow-only device buffer of matched_points
  // matched_edges: grow-only device buffers (the visits staged per trace, the per-trace counts /
  // offsets / totals, the compacted visits, the shapes), its events and the last call's sizes
  DevBuf<char> me_stage_, me_small_, me_edges_, me_shape_;
  PartTimer me_timer_;
  uint32_t me_traces_ = 0;
  uint64_t me_n_ = 0, me_v_ = 0;
  double me_ms_ = 0.0;
  bool me_ran_ = false;
  Workspace ws_;
  uint32_t n_traces_ = 0;
  uint64_t n_points_ = 0, n_trans_ = 0, n_path_ = 0, seg_used_ = 0;
  uint32_t timing_mask_ = 0;   // stages timed by HIP events
  bool has_report_ = false;
  bool isolate_ = false;
  int locality_ = -1;
  bool batch_sparse_ = false;     // the last run()'s batch is sampled sparsely (kLocalitySparseS)
  bool locality_used_ = false;
  void ensure_sort(uint64_t n);
  uint32_t err_bits_ = 0;
  PinBuf<uint32_t> hctl_;     // pinned host mirror of the control words
  StageBufs sb_;
  std::shared_ptr<LineState> ls_;
  int input_coding_ = 0;      // rule 20 (set_input_coding)
  bool skip_bad_chunks_ = false;
  bool from_points_ = false;
  uint32_t mode_mask_ = 0;   // travel modes of the batch (bit per Mode): which route balls K2 needs
  uint32_t turn_mask_ = 0;   // modes of the batch with a turn_penalty_factor > 0: turn rows, route_d
  float batch_radius_ = 0.f; // the batch's largest search_radius (m): K1's grid (Engine::k1_grid)
  void ensure_points(uint64_t n, uint32_t n_uuids, uint32_t n_opts);
  void ensure_rows(uint64_t n, uint32_t traces);
  PartTimer timer_;           // the stages timed by HIP events (timing_mask_), harvested by sync()
  double kms_[kNumKernels] = {0};
  uint64_t klaunch_[kNumKernels] = {0};
};

// K1's grid refinement for a graph (host only; engine.hip): each graph-file cell split f x f
uint32_t choose_grid_split(const Graph& g);
// the same for queries of radius_m (the padded box of that radius)
uint32_t choose_grid_split_for(const Graph& g, float radius_m);

// one K1 grid in HBM: its cell ranges, self-contained cell records and geometry
struct K1Grid {
  const uint32_t* cell_off = nullptr;
  const uint4* cell_rec = nullptr;
  double lon0 = 0, lat0 = 0, dlon = 0, dlat = 0;
  uint32_t ncx = 0, ncy = 0, split = 1;
};

class Engine {
 public:
  Engine(const Graph& g, int device);
  ~Engine();
  Engine(const Engine&) = delete;
  Engine& operator=(const Engine&) = delete;
  const DevGraph& dev() const { return dg_; }
  // copy of the device view taken under the ball lock (tables may be added concurrently)
  DevGraph dev_snapshot() const;
  int device() const { return device_; }
  const Graph& host() const { return host_; }
  uint32_t n_segments() const { return host_.num_segments(); }
  // build (once) the route balls of every mode in `mode_mask` (bit per Mode); thread-safe
  void ensure_balls(uint32_t mode_mask);
  // build (once) the turn rows of the built tables of every mode in `mode_mask`; thread-safe
  void ensure_turn_rows(uint32_t mode_mask);
  uint32_t turn_row_mask() const { return dg_.ball_turn_mask; }
  double turn_build_ms(int mode) const { return mode >= 0 && mode <= kModePedestrian ? turn_ms_[mode] : 0.0; }
  // ball radius in cm for modes built from now on (0 disables the ball tier)
  void set_ball_radius(uint32_t radius_cm);
  uint32_t ball_radius() const { return ball_radius_cm_; }
  // stats of one mode's tables: {keys, table entries, nodes without a table, build ms}
  void ball_stats(int mode, double* out4) const;
  // radius (cm) the mode's tables were built at (0: none; its transitions use the search tiers)
  uint32_t mode_ball_radius(int mode) const;
  // modes whose tables were built on the GPU (bit per Mode)
  uint32_t ball_gpu_mask() const { return ball_gpu_; }
  // keys[2i], keys[2i+1] from node from[i] to road[i]'s node0 / node1 through the built tables
  // of `mode`, probed on the device as K2 does (all-ones: outside the ball / no table)
  void ball_lookup(int mode, uint64_t n, const uint32_t* from, const uint32_t* road, uint64_t* keys, uint8_t* preds);
  // K1's grid: each cell of the graph's grid split f x f (1 = the graph's grid)
  uint32_t grid_split() const { return grid_split_; }
  // K1's grid for a batch whose largest query radius is radius_m: the default one, or a second
  // split built when wider queries read fewer items on it (grid_alt_radius() and up)
  void k1_grid(float radius_m, DevGraph& g) const;
  uint32_t grid_alt_split() const { return n_grids_ > 1 ? grids_[1].split : 0u; }
  float grid_alt_radius() const { return grid_alt_radius_; }
  // locality order by default (Matcher::set_locality -1): graphs whose route tables and cell
  // records outgrow the L2s; and the shift from K1 grid cells to the coarse sort cells (~500 m)
  bool locality_default() const { return locality_default_; }
  uint32_t locality_shift() const { return locality_shift_; }
  uint32_t locality_bits() const { return locality_bits_; }
  // per road its first shape vertex (R + 1 words) in HBM, uploaded on first use: only the
  // matched-points stage walks a road's shape by road id (K1 reads cell records); thread-safe
  const uint32_t* road_vert_off_dev();

 private:
  int device_;
  Graph host_;
  DevGraph dg_{};
  std::vector<DevBuf<char>> allocs_;   // the graph's arrays, uploaded by the constructor
  DevBuf<uint2> ball_hdr_[5], ball_turn_[5];   // per mode the route balls and turn rows built later
  DevBuf<uint4> ball_ent_[5];                  // (a twin mode shares its twin's: dg_ alone names them)
  mutable std::mutex ball_mu_;
  uint32_t ball_radius_cm_ = 40000;   // set from auto_ball_radius_cm(graph) at construction
  uint32_t ball_built_ = 0;             // mode bits
  uint32_t ball_gpu_ = 0;               // mode bits built on the GPU
  uint32_t grid_split_ = 1;
  K1Grid grids_[2];
  int n_grids_ = 1;
  float grid_alt_radius_ = 0.f;         // batches with a query radius from this take grids_[1]
  bool locality_default_ = false;
  uint32_t locality_shift_ = 0, locality_bits_ = 0;
  uint64_t ball_bytes_ = 0;             // bytes of the tables built so far (all modes)
  uint32_t turn_tried_ = 0;             // modes whose turn rows were attempted (ensure_turn_rows)
  double turn_ms_[5] = {};
  bool build_balls_gpu(int mode, uint32_t radius_cm, uint32_t max_keys, uint64_t avail_bytes);
  double ball_info_[5][4] = {};
  DevBuf<uint32_t> road_vert_off_;
};

}  // namespace rm
