// capi.cpp — the extern "C" boundary of libreporter_match.so (include/reporter_match.h).
//
// Drop-in for the Python `valhalla` binding the reference calls:
//   valhalla.Configure      reference py/reporter_service.py:284, py/simple_reporter.py:132
//   valhalla.SegmentMatcher reference py/reporter_service.py:52,  py/simple_reporter.py:133
//   SegmentMatcher.Match    reference py/reporter_service.py:240, py/simple_reporter.py:166
// Match's reply follows the schema the reference documents at README.md:288-301
// and consumes at py/reporter_service.py:79-179.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <atomic>
#include <sys/resource.h>
#include <cctype>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <deque>
#include <thread>
#include <vector>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>

#include "../../include/reporter_match.h"
#include "engine.hpp"
#include "graph.hpp"
#include "host_pool.hpp"
#include "inflate.hpp"
#include "inflate_core.hpp"
#include "edges_json.hpp"
#include "json.hpp"
#include "osm_model.hpp"
#include "serve_policy.hpp"
#include "snapshot.hpp"
#include "trace_json.hpp"

using namespace rm;

static_assert(sizeof(rm_options) == sizeof(MatchOptions), "rm_options layout");
static_assert(sizeof(ReportStats) == 40, "ReportStats layout");

namespace {

thread_local std::string g_err;
int g_device = 0;

struct ParsedTrace;
class Coalescer;

struct Config {
  std::shared_ptr<Engine> engine;
  MatchOptions mode_defaults[5];
  std::unique_ptr<Coalescer> coalescer;   // request coalescing for concurrent Match calls
  ~Config();
};
std::mutex g_mu;
std::shared_ptr<Config> g_conf;

int fail(const std::string& m) {
  g_err = m;
  return 1;
}

template <class F>
int guarded(F&& f) {
  try {
    f();
    return 0;
  } catch (const std::exception& e) {
    return fail(e.what());
  } catch (...) {
    return fail("unknown error");
  }
}

int mode_from_name(const std::string& s) {
  if (s == "auto") return kModeAuto;
  if (s == "bus") return kModeBus;
  if (s == "motor_scooter") return kModeMotorScooter;
  if (s == "bicycle") return kModeBicycle;
  if (s == "pedestrian") return kModePedestrian;
  throw std::runtime_error("unsupported mode: " + s);
}
const char* kModeNames[5] = {"auto", "bus", "motor_scooter", "bicycle", "pedestrian"};

void apply_options(const json::Value* o, MatchOptions& m) {
  if (!o || o->type != json::Value::Object) return;
  auto num = [&](const char* k, float& dst) {
    const json::Value* v = o->get(k);
    if (v && v->is_num()) dst = (float)v->num;
    else if (v && v->type != json::Value::Null) throw std::runtime_error(std::string("match option ") + k + " must be a number");
  };
  num("sigma_z", m.sigma_z);
  num("beta", m.beta);
  num("search_radius", m.search_radius);
  num("gps_accuracy", m.gps_accuracy);
  num("breakage_distance", m.breakage_distance);
  num("interpolation_distance", m.interpolation_distance);
  num("max_route_distance_factor", m.max_route_distance_factor);
  num("max_route_time_factor", m.max_route_time_factor);
  num("turn_penalty_factor", m.turn_penalty_factor);
  if (!(m.sigma_z > 0.f) || !std::isfinite(m.sigma_z)) throw std::runtime_error("sigma_z must be positive");
  if (!(m.beta > 0.f) || !std::isfinite(m.beta)) throw std::runtime_error("beta must be positive");
  if (!(m.search_radius >= 0.f)) throw std::runtime_error("search_radius must be non-negative");
}

std::string dir_of(const std::string& p) {
  const size_t k = p.find_last_of('/');
  return k == std::string::npos ? std::string(".") : p.substr(0, k);
}

std::string read_file(const std::string& path) {
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) throw std::runtime_error("cannot open " + path);
  std::string s;
  char buf[65536];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, n);
  std::fclose(f);
  return s;
}

// parsed trace ready for the engine (one request of the coalesced path)
struct ParsedTrace {
  tj::PointSink pts;
  MatchOptions opt;
  // a Report request (DESIGN.md §3 rule 19): its threshold and level masks
  bool report = false;
  double threshold = 0.0;
  uint32_t rmask = 0, tmask = 0;
  // requests of one kind (and, for Report, one threshold) share a coalesced batch
  bool same_kind(const ParsedTrace& o) const { return report == o.report && (!report || threshold == o.threshold); }
};

// one /report Match request (trace_json.hpp: single validating pass, the DOM reader's contract)
ParsedTrace parse_trace(const char* text, const Config& conf) {
  ParsedTrace t;
  t.opt = tj::parse_request(text, conf.mode_defaults, t.pts);
  return t;
}

void check_threshold(double threshold_sec) {
  if (!std::isfinite(threshold_sec)) throw std::runtime_error("threshold_sec must be finite");
}

// one /report request whose whole reply the library writes (rm_report)
ParsedTrace parse_report_trace(const char* text, const Config& conf, double threshold_sec) {
  ParsedTrace t;
  tj::ReportLevels lv;
  t.opt = tj::parse_report_request(text, std::strlen(text), conf.mode_defaults, t.pts, lv);
  t.report = true;
  t.threshold = threshold_sec;
  t.rmask = lv.report_mask;
  t.tmask = lv.transition_mask;
  return t;
}

// Request coalescing (HTTP front end): the reference's service answers
// each /report on its own worker thread with its own matcher (py/reporter_service.py:28-64,
// 240).  Here every thread's Match is parsed on the calling thread, queued, and a single
// dispatcher thread runs whatever is queued as ONE GPU batch; requests that arrive while a
// batch runs form the next one, so nothing waits for a timer at low load and the batch
// grows with the load (optionally held open for window_ms to fill).  Each caller gets its
// own segments or its own error; the Java caller's 10 s socket timeout
// (HttpClient.java:80-87) bounds the useful batch size, not the GPU.
struct MatchRequest {
  ParsedTrace* trace;
  std::string out, err;
  // a dispatched request's segments: its caller formats the reply itself after the batch (the
  // dispatcher moves on to the next batch instead of formatting tens of replies)
  std::vector<SegmentRec> segs;
  std::vector<ReportRec> reps;   // (a Report request: its reports and stats too)
  ReportStats stats{};
  bool raw = false;
  bool done = false;
  void format() {
    if (trace->report) reply_format_one(segs.data(), (uint32_t)segs.size(), reps.data(), (uint32_t)reps.size(), stats, out);
    else tj::format_segments(segs.data(), (uint32_t)segs.size(), out);
  }
  // its caller waits here alone, on the request's own mutex: a batch's callers wake without
  // queueing on the coalescer's lock (at 256 clients that convoy cost ~0.1 ms of CPU per request)
  std::mutex mu;
  std::condition_variable cv;
};

void serve_batch(std::unique_ptr<Matcher>& m, Engine* eng, const std::vector<MatchRequest*>& batch, double* tm,
                 bool defer_format = false);

class Coalescer {
 public:
  // `workers` dispatcher threads, each with its own Matcher (workspace + HIP stream): while one
  // batch runs on the GPU or is being formatted, the next one collects and starts on another
  Coalescer(std::shared_ptr<Engine> e, double window_ms, size_t max_traces, int workers)
      : eng_(std::move(e)), window_ms_(window_ms), max_(max_traces ? max_traces : 1) {
    for (int i = 0; i < std::max(1, workers); ++i) th_.emplace_back([this] { loop(); });
  }
  ~Coalescer() {
    {
      std::lock_guard<std::mutex> lk(mu_);
      stop_ = true;
    }
    cv_req_.notify_all();
    for (auto& t : th_) t.join();
  }
  // own: the caller allows the inline path.  While the service runs one request at a time (the last
  // kLoneStreak batches each held a single request) and is idle now, a request runs on its
  // caller's thread (on the coalescer's single inline matcher) through the same serve_batch: two thread hand-offs fewer on a
  // lone caller's latency (C1).  Under concurrent load batches hold many requests, the streak
  // is broken and every request queues (running requests inline there split the batches: 60-point
  // requests at 64 clients 7.6 -> 5.9 M points/s when any idle moment went inline).
  std::string submit(ParsedTrace* t, std::unique_ptr<Matcher>* own = nullptr) {
    MatchRequest r;
    r.trace = t;
    bool here = false;
    {
      std::lock_guard<std::mutex> lk(mu_);
      if (stop_) throw std::runtime_error("matcher is shutting down");
      if (own && inline_ok() && lone_ >= kLoneStreak && q_.empty() && busy_ == 0 && inline_ == 0) {
        here = true;
        ++inline_;
        ++batches_;
        ++requests_;
        max_seen_ = std::max<uint64_t>(max_seen_, 1);
      } else {
        q_.push_back(&r);
      }
    }
    if (here) {
      double tm[4] = {0, 0, 0, 0};
      const std::vector<MatchRequest*> one{&r};
      // on the coalescer's one inline matcher (inline_ == 1 here, so no other request uses it):
      // callers do not each keep a workspace, pinned buffers and a stream for their one inline run
      serve_batch(inline_m_, eng_.get(), one, tm);   // fills r.out / r.err (serve_policy.hpp)
      {
        std::lock_guard<std::mutex> lk(mu_);
        --inline_;
        for (int i = 0; i < 4; ++i) tm_[i] += tm[i];
      }
      if (!r.err.empty()) throw std::runtime_error(r.err);
      return std::move(r.out);
    }
    cv_req_.notify_one();
    {
      std::unique_lock<std::mutex> lk(r.mu);
      r.cv.wait(lk, [&] { return r.done; });
    }
    if (!r.err.empty()) throw std::runtime_error(r.err);
    if (r.raw) r.format();
    return std::move(r.out);
  }
  void stats(uint64_t out[4]) {
    std::lock_guard<std::mutex> lk(mu_);
    out[0] = batches_; out[1] = requests_; out[2] = max_seen_; out[3] = (uint64_t)q_.size();
  }
  void timing(double out[4]) {
    std::lock_guard<std::mutex> lk(mu_);
    for (int i = 0; i < 4; ++i) out[i] = tm_[i];
  }

 private:
  void loop();
  std::shared_ptr<Engine> eng_;
  double window_ms_;
  size_t max_;
  std::mutex mu_;
  std::condition_variable cv_req_;
  std::deque<MatchRequest*> q_;
  bool stop_ = false;
  static constexpr int kLoneStreak = 8;
  static bool fmt_callers() {   // RM_COALESCE_FORMAT=dispatcher: the dispatcher formats the replies (A/B)
    static const bool on = [] { const char* e = std::getenv("RM_COALESCE_FORMAT"); return !(e && std::strcmp(e, "dispatcher") == 0); }();
    return on;
  }
  static double trace_ms() {   // RM_COALESCE_TRACE=<ms>: a batch slower than that is printed to stderr
    static const double v = [] { const char* e = std::getenv("RM_COALESCE_TRACE"); return e && *e ? std::strtod(e, nullptr) : 0.0; }();
    return v;
  }
  static bool inline_ok() {   // RM_COALESCE_INLINE=0: every request queues (A/B)
    static const bool on = [] { const char* e = std::getenv("RM_COALESCE_INLINE"); return !(e && *e == '0'); }();
    return on;
  }
  int busy_ = 0, inline_ = 0;   // dispatchers running a batch; requests running on their caller's thread
  int lone_ = 0;                // consecutive dispatched batches of one request
  uint64_t batches_ = 0, requests_ = 0, max_seen_ = 0;
  double tm_[4] = {0, 0, 0, 0};   // dispatcher wall ms: staging, engine, download, formatting
  std::vector<std::thread> th_;
  std::unique_ptr<Matcher> inline_m_;   // the lone caller's runs (created on the first; guarded by inline_)
};

Config::~Config() { coalescer.reset(); }

char* dup_string(const std::string& s) {
  char* p = (char*)std::malloc(s.size() + 1);
  if (!p) throw std::bad_alloc();
  std::memcpy(p, s.c_str(), s.size() + 1);
  return p;
}

// pinned host staging of one matcher's batch arrays (grow-only): the parse threads copy their
// points here and the engine's uploads run at full PCIe rate
struct HostStaging {
  PinBuf<float> lon, lat, acc;
  PinBuf<double> time;
  size_t cap = 0;
  void ensure(size_t n) {
    if (n <= cap) return;
    const size_t c = std::max(n + n / 4, cap + cap / 2) + 4096;
    cap = 0;
    lon.reset(); lat.reset(); acc.reset(); time.reset();   // all four go before the first is taken again
    lon.reserve(c); lat.reserve(c); acc.reserve(c); time.reserve(c);
    cap = c;
  }
};

// pageable staging of a small batch's arrays (grow-only, geometric)
struct PageableStaging {
  std::vector<float> lon, lat, acc;
  std::vector<double> time;
  void ensure(size_t n) {
    if (n <= lon.size()) return;
    const size_t c = std::max<size_t>(n, 2 * lon.size()) + 1024;
    lon.resize(c); lat.resize(c); acc.resize(c); time.resize(c);
  }
};

// run a list of parsed traces as one batch on matcher m; per-trace JSON replies, and per-trace
// error messages (non-empty = that trace failed alone; its reply is empty)
// fn(i) for i in [0, n) over the host pool (up to 16 threads) in contiguous chunks (the JSON
// parse and formatting around a batch are host work that a single thread makes the boundary's
// limit); an exception is rethrown for the lowest failing index's chunk, as a serial loop would
template <class F>
void parallel_for(size_t n, F&& fn, size_t per = 32) {
  HostPool& pool = HostPool::get();
  const size_t nt = std::min<size_t>(pool.size(), (n + per - 1) / per);
  if (nt <= 1) {
    for (size_t i = 0; i < n; ++i) fn(i);
    return;
  }
  pool.run(nt, [&](size_t t) {
    const size_t a = n * t / nt, b = n * (t + 1) / nt;
    for (size_t i = a; i < b; ++i) fn(i);
  });
}

// tm (may be null) accumulates host wall ms: [0] staging, [1] engine run, [2] segment download,
// [3] reply formatting
// raw (optional): each trace's segments instead of its formatted reply (the coalescer's callers
// format their own)
struct RawRecords {   // per trace: its segments and, for a Report batch, its reports and stats
  std::vector<std::vector<SegmentRec>> segs;
  std::vector<std::vector<ReportRec>> reps;
  std::vector<ReportStats> stats;
};
std::vector<std::string> match_parsed(Matcher& m, const std::vector<ParsedTrace*>& pt, std::vector<std::string>* errs,
                                      double* tm = nullptr, RawRecords* raw = nullptr) {
  using clk = std::chrono::steady_clock;
  auto ms_since = [](clk::time_point a) { return std::chrono::duration<double, std::milli>(clk::now() - a).count(); };
  clk::time_point t0 = clk::now();
  const size_t n = pt.size();
  std::vector<uint32_t> off(n + 1, 0), topt(n);
  std::vector<MatchOptions> opts(n);
  for (size_t i = 0; i < n; ++i) { off[i + 1] = off[i] + (uint32_t)pt[i]->pts.size(); opts[i] = pt[i]->opt; topt[i] = (uint32_t)i; }
  const uint64_t P = off[n];
  // a large batch goes up from this thread's pinned staging (grow-only): its uploads run as DMA
  // instead of staged pageable copies.  A small one (a coalesced service batch) is packed into the
  // matcher's own pinned block by Matcher::run, so it stages in pageable memory here: no pinned
  // allocation (and no pool hand-off) on a caller's thread (the inline path), and none freed when
  // that thread exits.
  constexpr uint64_t kPinnedStagingMin = 65536;   // Matcher::run's small-run limit (RM_SMALL_BATCH_POINTS)
  float *lon, *lat, *acc;
  double* time;
  if (P > kPinnedStagingMin) {
    static thread_local HostStaging staging;
    staging.ensure(P);
    lon = staging.lon; lat = staging.lat; acc = staging.acc; time = staging.time;
  } else {
    static thread_local PageableStaging staging;
    staging.ensure(P);
    lon = staging.lon.data(); lat = staging.lat.data(); acc = staging.acc.data(); time = staging.time.data();
  }
  auto stage = [&](size_t i) {
    const tj::PointSink& q = pt[i]->pts;
    std::copy(q.lon.begin(), q.lon.end(), lon + off[i]);
    std::copy(q.lat.begin(), q.lat.end(), lat + off[i]);
    std::copy(q.acc.begin(), q.acc.end(), acc + off[i]);
    std::copy(q.time.begin(), q.time.end(), time + off[i]);
  };
  if (P > kPinnedStagingMin) parallel_for(n, stage);   // (a small batch copies in microseconds: no pool hand-off)
  else for (size_t i = 0; i < n; ++i) stage(i);
  HostBatch hb;
  hb.n_traces = (uint32_t)n; hb.trace_off = off.data(); hb.lon = lon; hb.lat = lat;
  hb.time = time; hb.accuracy = acc; hb.n_opts = (uint32_t)n; hb.opts = opts.data();
  hb.trace_opt = topt.data();
  const bool report = n && pt[0]->report;   // (a batch is of one kind: Coalescer::loop)
  std::vector<uint32_t> rmask, tmask;
  RunParams rp;
  rp.do_report = 0;
  rp.prefetch_segments = 1;   // the replies are the segments: a small run readies them itself
  if (report) {
    rmask.resize(n); tmask.resize(n);
    for (size_t i = 0; i < n; ++i) { rmask[i] = pt[i]->rmask; tmask[i] = pt[i]->tmask; }
    rp.do_report = 1;
    rp.threshold_sec = pt[0]->threshold;
    rp.trace_report_mask = rmask.data();
    rp.trace_transition_mask = tmask.data();
    rp.prefetch_reports = 1;   // ... and the reports and stats
  }
  m.set_isolation(true);
  if (tm) { tm[0] += ms_since(t0); t0 = clk::now(); }
  m.run(hb, rp);
  if (tm) { tm[1] += ms_since(t0); t0 = clk::now(); }
  std::vector<uint32_t> terr(n, 0u);
  if (m.error_bits()) m.get_trace_errors(terr.data());
  std::vector<uint32_t> soff, rbase, rcnt;
  std::vector<SegmentRec> segs;
  std::vector<ReportRec> reps;
  std::vector<ReportStats> stats;
  if (report) m.get_report_records(soff, segs, rbase, rcnt, reps, stats);
  else m.get_segments(soff, segs);
  if (tm) { tm[2] += ms_since(t0); t0 = clk::now(); }
  std::vector<std::string> out(n);
  if (errs) errs->assign(n, std::string());
  for (size_t i = 0; i < n; ++i) {
    if (!terr[i]) continue;
    if (!errs) throw std::runtime_error("trace " + std::to_string(i) + ": " + error_text(terr[i]));
    (*errs)[i] = error_text(terr[i]);
  }
  if (raw) {
    raw->segs.resize(n);
    if (report) { raw->reps.resize(n); raw->stats = stats; }
    for (size_t i = 0; i < n; ++i) {
      if (terr[i]) continue;
      raw->segs[i].assign(segs.data() + soff[i], segs.data() + soff[i + 1]);
      if (report) raw->reps[i].assign(reps.data() + rbase[i], reps.data() + rbase[i] + rcnt[i]);
    }
    if (tm) tm[3] += ms_since(t0);
    return out;
  }
  // replies of a coalesced batch (tens of requests, ~10 us each) over the pool in chunks of 4
  parallel_for(n, [&](size_t i) {
    if (terr[i]) return;
    if (report) reply_format_one(segs.data() + soff[i], soff[i + 1] - soff[i], reps.data() + rbase[i], rcnt[i], stats[i], out[i]);
    else tj::format_segments(segs.data() + soff[i], soff[i + 1] - soff[i], out[i]);
  }, 4);
  if (tm) tm[3] += ms_since(t0);
  return out;
}

// Run `batch` and fill each request's reply or error.  A failure that belongs to one trace is
// reported per trace by the engine; a whole-batch failure follows serve_policy.hpp: a batch too
// large for the device is retried by halves (bounded), any other error fails every request in
// it at once.  A failed run drops the matcher, so what follows starts on a fresh workspace.
void serve_batch(std::unique_ptr<Matcher>& m, Engine* eng, const std::vector<MatchRequest*>& batch, double* tm,
                 bool defer_format) {
  int budget = kServeRetryBudget;
  auto run = [&](MatchRequest* const* reqs, size_t n) {
    try {
      if (!m) m = std::make_unique<Matcher>(eng);
      std::vector<ParsedTrace*> pt(n);
      for (size_t i = 0; i < n; ++i) pt[i] = reqs[i]->trace;
      std::vector<std::string> errs;
      RawRecords raw;
      std::vector<std::string> outs = match_parsed(*m, pt, &errs, tm, defer_format ? &raw : nullptr);
      for (size_t i = 0; i < n; ++i) {
        if (!errs[i].empty()) {
          reqs[i]->err = errs[i];
        } else if (defer_format) {
          reqs[i]->segs = std::move(raw.segs[i]);
          if (pt[i]->report) { reqs[i]->reps = std::move(raw.reps[i]); reqs[i]->stats = raw.stats[i]; }
          reqs[i]->raw = true;
        } else {
          reqs[i]->out = std::move(outs[i]);
        }
      }
    } catch (...) {
      m.reset();
      throw;
    }
  };
  auto fail = [](MatchRequest* r, const char* msg) { r->err = msg; };
  serve_split(batch.data(), batch.size(), run, fail, budget);
}

void Coalescer::loop() {
  std::unique_ptr<Matcher> m;
  uint64_t traced = 0;
  for (;;) {
    std::vector<MatchRequest*> batch;
    {
      std::unique_lock<std::mutex> lk(mu_);
      cv_req_.wait(lk, [&] { return stop_ || !q_.empty(); });
      if (q_.empty() && stop_) break;
      if (window_ms_ > 0) {
        const auto until = std::chrono::steady_clock::now() + std::chrono::microseconds((int64_t)(window_ms_ * 1000));
        while (!stop_ && q_.size() < max_ && cv_req_.wait_until(lk, until) != std::cv_status::timeout) {}
      }
      // a batch holds requests of one kind: the first of another kind waits for the next batch (a
      // Match reply is never made by a run with reporting on)
      while (!q_.empty() && batch.size() < max_ && (batch.empty() || q_.front()->trace->same_kind(*batch[0]->trace))) {
        batch.push_back(q_.front());
        q_.pop_front();
      }
      batches_++;
      requests_ += batch.size();
      max_seen_ = std::max<uint64_t>(max_seen_, batch.size());
      lone_ = batch.size() == 1 ? lone_ + 1 : 0;
      ++busy_;
      if (!q_.empty()) cv_req_.notify_one();   // (the other kind's requests: another dispatcher may take them now)
    }
    double tm[4] = {0, 0, 0, 0};
    serve_batch(m, eng_.get(), batch, tm, fmt_callers());   // out / err (or segs) of each request, not under the lock
    if (trace_ms() > 0) {
      if (tm[0] + tm[1] + tm[2] + tm[3] > trace_ms())
        std::fprintf(stderr, "coalesce: batch of %zu requests: staging %.3f engine %.3f download %.3f format %.3f ms\n",
                     batch.size(), tm[0], tm[1], tm[2], tm[3]);
      if (++traced % 1024 == 0) {   // this dispatcher's own CPU time so far
        rusage u{};
        getrusage(RUSAGE_THREAD, &u);
        std::fprintf(stderr, "coalesce: dispatcher after %llu batches: cpu %.3f s (user %.3f)\n", (unsigned long long)traced,
                     u.ru_utime.tv_sec + u.ru_utime.tv_usec * 1e-6 + u.ru_stime.tv_sec + u.ru_stime.tv_usec * 1e-6,
                     u.ru_utime.tv_sec + u.ru_utime.tv_usec * 1e-6);
      }
    }
    {
      std::lock_guard<std::mutex> lk(mu_);
      --busy_;
      for (int i = 0; i < 4; ++i) tm_[i] += tm[i];
    }
    for (MatchRequest* r : batch) {
      std::lock_guard<std::mutex> lk(r->mu);
      r->done = true;
      r->cv.notify_one();   // under its lock: the request (and its cv) lives until its caller returns
    }
  }
}

}  // namespace

// a pinned host buffer, grow-only
struct PinnedBytes {
  PinBuf<char> p;
  size_t cap = 0;
  void ensure(size_t n) {
    if (n <= cap && p) return;
    cap = 0;
    const size_t c = std::max<size_t>(n + n / 4, 1u << 16);
    p.reserve(c);
    cap = c;
  }
};

struct rm_matcher {
  std::shared_ptr<Config> conf;
  std::unique_ptr<Matcher> m;
  HostStaging stage;
  std::vector<tj::PointSink> sinks;   // per parse thread, grow-only (no page faults on a warm matcher)
  std::vector<PinnedBytes> arenas;    // per parse thread: trace-array bytes for the device parser
  ReplyWriter reply;                  // rm_report_batch*: the device writer's buffers (grow-only)
  double ms[6] = {};   // the last rm_match_batch / rm_report_batch: parse, stage, engine, download, format, total
  uint64_t reply_info[4] = {};   // the last rm_report_batch: reply bytes, flagged traces, writer (1 host, 2 device), device us
};

namespace {

// The reply side of rm_match_batch (both parsers): per-trace failures fail the call naming the
// trace, then the segments come down once and each pool thread formats its range of replies
// straight into the caller's output strings.
// replies packed into one buffer (rm_match_batch_packed): reply i is (*buf)[off[i], off[i+1])
struct PackedOut {
  char** buf;
  uint64_t* off;
};

// the request's points of a batch whose replies also carry matched_points (rm_match_points*):
// trace i's points are lon / lat [off[i], off[i+1])
struct PointsIn {
  const float* lon;
  const float* lat;
  const uint32_t* off;
};

// what makes a batch call a Report call (rm_report_batch*): the call's threshold and, filled by the
// structure read, every request's level masks
struct ReportCall {
  double threshold = 15.0;
  std::vector<uint32_t> rmask, tmask;
  void params(RunParams& rp) const {
    rp.do_report = 1;
    rp.threshold_sec = threshold;
    rp.trace_report_mask = rmask.data();
    rp.trace_transition_mask = tmask.data();
  }
};

// one request of a batch call, as Match or as Report reads it (span: left to the device parser)
MatchOptions parse_batch_request(const char* text, size_t len, const Config& conf, tj::PointSink& sk, tj::TraceSpan* span,
                                 ReportCall* rc, size_t i) {
  if (!rc) return span ? tj::parse_request_deferred(text, len, conf.mode_defaults, sk, *span) : tj::parse_request(text, len, conf.mode_defaults, sk);
  tj::ReportLevels lv;
  const MatchOptions o = tj::parse_report_request(text, len, conf.mode_defaults, sk, lv, span);
  rc->rmask[i] = lv.report_mask;
  rc->tmask[i] = lv.transition_mask;
  return o;
}

// The reply side of rm_report_batch*: per-trace failures fail the call naming the trace; a run
// above the small-run limit (RM_REPLY_DEVICE_MIN_POINTS) has its replies written on the device and
// downloads text and offsets straight into the packed buffer, a smaller one downloads the records
// and the host writer formats them.  Both give the same bytes.
void finish_report_batch(rm_matcher* m, Matcher& mt, size_t n, uint64_t points, char** outs, const PackedOut* pk) {
  using clk = std::chrono::steady_clock;
  auto ms_since = [](clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); };
  std::vector<uint32_t> terr(n, 0u);
  if (mt.error_bits()) mt.get_trace_errors(terr.data());
  for (size_t i = 0; i < n; ++i)
    if (terr[i]) throw std::runtime_error("trace " + std::to_string(i) + ": " + error_text(terr[i]));
  std::vector<uint64_t> own_off;
  uint64_t* off = pk ? pk->off : (own_off.resize(n + 1), own_off.data());
  char* buf = nullptr;
  uint64_t flagged = 0;
  const auto t3 = clk::now();
  if (points > reply_device_min_points()) {
    double dev_ms = 0.0;
    m->reply.write(mt.device(), mt.stream(), mt.reply_source(), &buf, off, &flagged, &dev_ms);
    m->ms[4] = dev_ms;                                   // the writer's kernels and scans
    m->ms[3] = std::max(0.0, ms_since(t3) - dev_ms);     // the downloads (and the host's share)
    m->reply_info[2] = 2; m->reply_info[3] = (uint64_t)(dev_ms * 1000.0 + 0.5);
  } else {
    std::vector<uint32_t> soff, rbase, rcnt;
    std::vector<SegmentRec> segs;
    std::vector<ReportRec> reps;
    std::vector<ReportStats> stats;
    mt.get_report_records(soff, segs, rbase, rcnt, reps, stats);
    m->ms[3] = ms_since(t3);
    const auto t4 = clk::now();
    reply_format_host((uint32_t)n, soff.data(), segs.data(), rbase.data(), rcnt.data(), reps.data(), stats.data(), &buf, off, &flagged);
    m->ms[4] = ms_since(t4);
    m->reply_info[2] = 1; m->reply_info[3] = 0;
  }
  m->reply_info[0] = off[n]; m->reply_info[1] = flagged;
  if (pk) { *pk->buf = buf; return; }
  try {
    for (size_t i = 0; i < n; ++i) {
      const size_t k = (size_t)(off[i + 1] - off[i]);
      outs[i] = static_cast<char*>(std::malloc(k + 1));
      if (!outs[i]) throw std::bad_alloc();
      std::memcpy(outs[i], buf + off[i], k);
      outs[i][k] = 0;
    }
  } catch (...) {
    std::free(buf);
    throw;
  }
  std::free(buf);
}

void finish_json_batch(rm_matcher* m, Matcher& mt, size_t n, size_t nt, char** outs, const PackedOut* pk = nullptr,
                       const PointsIn* pin = nullptr, bool with_edges = false) {
  using clk = std::chrono::steady_clock;
  auto ms_since = [](clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); };
  std::vector<uint32_t> terr(n, 0u);
  if (mt.error_bits()) mt.get_trace_errors(terr.data());
  for (size_t i = 0; i < n; ++i)
    if (terr[i]) throw std::runtime_error("trace " + std::to_string(i) + ": " + error_text(terr[i]));
  const auto t3 = clk::now();
  std::vector<uint32_t> soff;
  std::vector<SegmentRec> segs;
  mt.get_segments(soff, segs);
  std::vector<MatchedPoint> mp;
  if (pin) {   // the matched-points stage runs here, on request, over what the run left in HBM
    mp.resize(pin->off[n]);
    mt.matched_points(mp.data());
  }
  // ... and so does the matched-edges stage (rm_match_edges*)
  std::vector<uint32_t> eoff, shoff;
  std::vector<MatchedEdge> me;
  std::vector<float> shape;
  if (with_edges) {
    uint64_t tot[2];
    mt.matched_edges(tot);
    eoff.resize(n + 1); shoff.resize(n + 1);
    me.resize(tot[0]); shape.resize(2 * tot[1]);
    mt.get_matched_edges(eoff.data(), me.data(), shoff.data(), shape.data());
  }
  m->ms[3] = ms_since(t3);
  const auto t4 = clk::now();
  if (pk) {   // each thread formats its range into one string, then they are copied into one buffer
    std::vector<std::string> part(nt);
    std::vector<uint64_t> len(n);
    HostPool::get().run(nt, [&](size_t t) {
      const size_t a = n * t / nt, b = n * (t + 1) / nt;
      part[t].reserve((size_t)(soff[b] - soff[a]) * 224 + (b - a) * 16);   // ~200 bytes per segment
      std::string js;
      for (size_t i = a; i < b; ++i) {
        tj::format_segments(segs.data() + soff[i], soff[i + 1] - soff[i], js);
        part[t] += js;
        len[i] = js.size();
      }
    });
    pk->off[0] = 0;
    for (size_t i = 0; i < n; ++i) pk->off[i + 1] = pk->off[i] + len[i];
    char* buf = static_cast<char*>(std::malloc(pk->off[n] + 1));
    if (!buf) throw std::bad_alloc();
    HostPool::get().run(nt, [&](size_t t) {
      std::memcpy(buf + pk->off[n * t / nt], part[t].data(), part[t].size());
    });
    buf[pk->off[n]] = 0;
    *pk->buf = buf;
  } else {
    HostPool::get().run(nt, [&](size_t t) {
      const size_t a = n * t / nt, b = n * (t + 1) / nt;
      std::string js;
      for (size_t i = a; i < b; ++i) {
        tj::format_segments(segs.data() + soff[i], soff[i + 1] - soff[i], js);
        if (pin) {
          const std::vector<EdgeRec>& edges = mt.engine().host().edges;
          const uint32_t o = pin->off[i];
          tj::append_matched_points(mp.data() + o, pin->off[i + 1] - o, pin->lon + o, pin->lat + o,
                                    [&](uint32_t e) { return edges[e].len_cm; }, js);
        }
        if (with_edges) {
          const std::vector<uint64_t>& seg_id = mt.engine().host().seg_id;
          tj::append_matched_edges(me.data() + eoff[i], eoff[i + 1] - eoff[i], shape.data() + 2 * (size_t)shoff[i],
                                   shoff[i + 1] - shoff[i], [&](uint32_t sd) { return seg_id[sd]; }, js);
        }
        outs[i] = dup_string(js);
      }
    });
  }
  m->ms[4] = ms_since(t4);
}

// rm_match_batch with the trace arrays parsed on the device (engine.hip k_parse_json).  Each pool
// thread reads its requests' structure on the host (parse_request_deferred) and copies their
// trace-array bytes into its pinned arena; the arenas go up in request order (one contiguous span
// per trace) and one wave per trace parses them into the workspace's point arrays.  A request the
// host did not defer (not a compact-looking trace) keeps its host-parsed points.  A trace the
// device flags is parsed again on the host.  Any failure, and a flagged trace whose point count
// differs from its '{' count, returns false before anything ran: the caller then takes the host
// path, which reports exactly the error the host reader gives.
// batches of fewer JSON bytes take the host parse (RM_JSON_DEVICE_MIN_MB, default 8; read per call)
uint64_t json_device_min_bytes() {
  const char* e = std::getenv("RM_JSON_DEVICE_MIN_MB");
  const double mb = e && *e ? std::strtod(e, nullptr) : 8.0;
  return (uint64_t)(std::max(0.0, mb) * 1048576.0);
}

bool match_json_batch_device(rm_matcher* m, const char* const* traces, size_t n, char** outs, const PackedOut* pk,
                             ReportCall* rc = nullptr) {
  using clk = std::chrono::steady_clock;
  auto ms_since = [](clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); };
  const auto t0 = clk::now();
  HostPool& pool = HostPool::get();
  const size_t nt = std::max<size_t>(1, std::min<size_t>(pool.size(), (n + 15) / 16));
  if (m->sinks.size() < nt) m->sinks.resize(nt);
  while (m->arenas.size() < nt) m->arenas.emplace_back();
  const Config& conf = *m->conf;
  if (!m->m) m->m = std::make_unique<Matcher>(conf.engine.get());
  Matcher& mt = *m->m;
  // the requests' lengths bound each thread's trace bytes: its region of the device buffer
  std::vector<size_t> len(n);
  std::vector<uint64_t> region(nt + 1, 0);
  pool.run(nt, [&](size_t t) {
    const size_t a = n * t / nt, b = n * (t + 1) / nt;
    uint64_t bytes = 0;
    for (size_t i = a; i < b; ++i) bytes += len[i] = std::strlen(traces[i]);
    region[t + 1] = (bytes + 15) & ~(uint64_t)15;
  });
  for (size_t t = 0; t < nt; ++t) region[t + 1] += region[t];
  // below a few MB the host threads parse faster than the device path's fixed cost (an upload, a
  // kernel and a read-back: ~0.5 ms for one 1,000-point request against ~0.1 ms on the host)
  if (region[nt] < json_device_min_bytes()) return false;
  mt.json_reserve_bytes(region[nt]);
  std::vector<uint32_t> cnt(n), topt(n);
  std::vector<uint64_t> span(2 * n, 0), sink_at(n, 0);
  std::vector<uint8_t> host_parsed(n, 0);
  std::vector<MatchOptions> opts(n);
  std::vector<char> failed(nt, 0);
  // each thread reads its requests' structure, copies their trace arrays into its pinned arena and
  // sends the arena at once, so the copies overlap the other threads' parsing
  pool.run(nt, [&](size_t t) {
    const size_t a = n * t / nt, b = n * (t + 1) / nt;
    PinnedBytes& ar = m->arenas[t];
    ar.ensure(region[t + 1] - region[t] + 1);
    tj::PointSink& sk = m->sinks[t];
    sk.clear();
    size_t at = 0;
    for (size_t i = a; i < b && !failed[t]; ++i) {
      topt[i] = (uint32_t)i;
      tj::TraceSpan sp;
      const size_t before = sk.size();
      try {
        opts[i] = parse_batch_request(traces[i], len[i], conf, sk, &sp, rc, i);
      } catch (const std::exception&) {
        try {
          sp = tj::TraceSpan();
          opts[i] = parse_batch_request(traces[i], len[i], conf, sk, nullptr, rc, i);
        } catch (const std::exception&) {
          failed[t] = 1;   // the host path reports it (as the first failing request)
          break;
        }
      }
      if (sp.on) {
        const size_t k = (size_t)(sp.e - sp.b);
        std::memcpy(ar.p + at, sp.b, k);
        span[2 * i] = region[t] + at;
        span[2 * i + 1] = region[t] + at + k;
        at += k;
        cnt[i] = sp.n_open;
      } else {
        host_parsed[i] = 1;
        sink_at[i] = before;
        cnt[i] = (uint32_t)(sk.size() - before);
      }
    }
    if (!failed[t]) mt.json_upload(region[t], ar.p, at);
  });
  for (size_t t = 0; t < nt; ++t)
    if (failed[t]) { mt.sync(); return false; }
  std::vector<uint32_t> off(n + 1, 0);
  for (size_t i = 0; i < n; ++i) {
    if ((uint64_t)off[i] + cnt[i] >= 0xffffffffull) throw BatchTooLarge("batch too large (points >= 2^32)");
    off[i + 1] = off[i] + cnt[i];
  }
  const uint64_t P = off[n];
  m->ms[0] = ms_since(t0);
  const auto t1 = clk::now();
  mt.json_reserve(P, (uint32_t)n, (uint32_t)n);
  std::vector<double> tsp(2 * n, 0.0);
  auto host_points = [&](size_t i, const tj::PointSink& sk, size_t at) {
    const size_t k = cnt[i];
    mt.upload_points(off[i], k, sk.lon.data() + at, sk.lat.data() + at, sk.time.data() + at, sk.acc.data() + at);
    if (k) { tsp[2 * i] = sk.time[at]; tsp[2 * i + 1] = sk.time[at + k - 1]; }
  };
  for (size_t t = 0; t < nt; ++t) {
    const size_t a = n * t / nt, b = n * (t + 1) / nt;
    for (size_t i = a; i < b; ++i)
      if (host_parsed[i]) host_points(i, m->sinks[t], sink_at[i]);
  }
  std::vector<uint32_t> flags(n, 0u);
  std::vector<double> dtsp(2 * n, 0.0);
  mt.json_parse(span.data(), off.data(), (uint32_t)n, flags.data(), dtsp.data());
  // one sink per flagged trace, alive until the run: their points go up with hipMemcpyAsync from
  // pageable memory, so none is reused or freed before the stream has consumed it
  std::deque<tj::PointSink> fixes;
  for (size_t i = 0; i < n; ++i) {
    if (host_parsed[i]) continue;
    if (!flags[i]) { tsp[2 * i] = dtsp[2 * i]; tsp[2 * i + 1] = dtsp[2 * i + 1]; continue; }
    // not the compact layout after all: the host reader's points, if they fit the trace's slots
    tj::PointSink& fix = fixes.emplace_back();
    try {
      opts[i] = parse_batch_request(traces[i], len[i], conf, fix, nullptr, rc, i);
    } catch (const std::exception&) {
      mt.sync();   // the uploads queued so far read host memory this function owns
      return false;
    }
    if (fix.size() != cnt[i]) { mt.sync(); return false; }
    host_points(i, fix, 0);
  }
  m->ms[1] = ms_since(t1);
  const auto t2 = clk::now();
  RunParams rp;
  rp.do_report = 0;
  if (rc) rc->params(rp);
  mt.set_isolation(true);
  mt.run_parsed(off.data(), (uint32_t)n, opts.data(), (uint32_t)n, topt.data(), tsp.data(), rp);
  m->ms[2] = ms_since(t2);
  if (rc) finish_report_batch(m, mt, n, P, outs, pk);
  else finish_json_batch(m, mt, n, nt, outs, pk);
  m->ms[5] = ms_since(t0);
  return true;
}

bool json_device_enabled() {
  static const bool on = [] {
    const char* e = std::getenv("RM_JSON_DEVICE");
    return !(e && *e == '0');
  }();
  return on;
}

// rm_match_batch without the coalescer: each pool thread parses a contiguous range of the
// requests into its own point arrays, copies them into the matcher's pinned staging at their
// batch offsets, and after the engine's run formats its range's replies straight into the
// caller's output strings.  Any failing trace fails the call, naming the trace.
// points: the replies also carry matched_points (rm_match_points*); the requests are then parsed
// on the host, whose staging keeps the input points an unmatched entry reports.
// edges: the replies also carry edges and shape (rm_match_edges*); parsed on the host likewise.
// rc: a Report call (rm_report_batch*): the level arrays are read with the structure, report() runs
// with the match and the replies are the complete /report bodies (finish_report_batch).
void match_json_batch(rm_matcher* m, const char* const* traces, size_t n, char** outs,
                      const PackedOut* pk = nullptr, bool points = false, bool edges = false, ReportCall* rc = nullptr) {
  if (rc) { rc->rmask.assign(n, 0u); rc->tmask.assign(n, 0u); }
  if (n && !points && !edges && json_device_enabled() && match_json_batch_device(m, traces, n, outs, pk, rc)) return;
  using clk = std::chrono::steady_clock;
  auto ms_since = [](clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); };
  const auto t0 = clk::now();
  HostPool& pool = HostPool::get();
  const size_t nt = std::max<size_t>(1, std::min<size_t>(pool.size(), (n + 15) / 16));
  if (m->sinks.size() < nt) m->sinks.resize(nt);
  std::vector<tj::PointSink>& sink = m->sinks;
  std::vector<uint32_t> cnt(n), topt(n);
  std::vector<size_t> len(n);
  std::vector<MatchOptions> opts(n);
  const Config& conf = *m->conf;
  pool.run(nt, [&](size_t t) {
    const size_t a = n * t / nt, b = n * (t + 1) / nt;
    size_t bytes = 0;
    for (size_t i = a; i < b; ++i) bytes += len[i] = std::strlen(traces[i]);
    tj::PointSink& sk = sink[t];
    sk.clear();
    const size_t guess = bytes / 48 + 16;   // a /report point is ~60-90 bytes of JSON
    sk.lon.reserve(guess); sk.lat.reserve(guess); sk.acc.reserve(guess); sk.time.reserve(guess);
    for (size_t i = a; i < b; ++i) {
      const size_t before = sk.size();
      opts[i] = parse_batch_request(traces[i], len[i], conf, sk, nullptr, rc, i);
      cnt[i] = (uint32_t)(sk.size() - before);
      topt[i] = (uint32_t)i;
    }
  });
  std::vector<uint32_t> off(n + 1, 0);
  for (size_t i = 0; i < n; ++i) {
    if ((uint64_t)off[i] + cnt[i] >= 0xffffffffull) throw BatchTooLarge("batch too large (points >= 2^32)");
    off[i + 1] = off[i] + cnt[i];
  }
  const uint64_t P = off[n];
  m->ms[0] = ms_since(t0);
  const auto t1 = clk::now();
  m->stage.ensure(P);
  HostStaging& hs = m->stage;
  pool.run(nt, [&](size_t t) {
    const size_t a = n * t / nt;
    const tj::PointSink& sk = sink[t];
    const size_t o = off[a], k = sk.size();
    std::memcpy(hs.lon + o, sk.lon.data(), k * 4);
    std::memcpy(hs.lat + o, sk.lat.data(), k * 4);
    std::memcpy(hs.acc + o, sk.acc.data(), k * 4);
    std::memcpy(hs.time + o, sk.time.data(), k * 8);
  });
  m->ms[1] = ms_since(t1);
  const auto t2 = clk::now();
  if (!m->m) m->m = std::make_unique<Matcher>(conf.engine.get());
  Matcher& mt = *m->m;
  HostBatch hb;
  hb.n_traces = (uint32_t)n; hb.trace_off = off.data(); hb.lon = hs.lon; hb.lat = hs.lat;
  hb.time = hs.time; hb.accuracy = hs.acc; hb.n_opts = (uint32_t)n; hb.opts = opts.data();
  hb.trace_opt = topt.data();
  RunParams rp;
  rp.do_report = 0;
  rp.prefetch_segments = 1;
  if (rc) { rc->params(rp); rp.prefetch_reports = 1; }
  mt.set_isolation(true);
  mt.run(hb, rp);
  m->ms[2] = ms_since(t2);
  const PointsIn pin{hs.lon, hs.lat, off.data()};
  if (rc) finish_report_batch(m, mt, n, P, outs, pk);
  else finish_json_batch(m, mt, n, nt, outs, pk, points ? &pin : nullptr, edges);
  m->ms[5] = ms_since(t0);
}

}  // namespace
struct rm_engine {
  std::shared_ptr<Engine> e;
};
struct rm_runner {
  std::shared_ptr<Engine> e;
  std::shared_ptr<Matcher> m;   // shared with the runner's sessions, which may outlive the handle
};

extern "C" {

const char* rm_last_error(void) { return g_err.c_str(); }
int rm_abi_version(void) { return RM_ABI_VERSION; }
int rm_set_device(int device) { g_device = device; return 0; }
int rm_device_count(int* count) {
  return guarded([&] { RM_HIP(hipGetDeviceCount(count)); });
}

void rm_default_options(rm_options* o) {
  const MatchOptions d = default_options();
  std::memcpy(o, &d, sizeof d);
}

int rm_configure(const char* conf_json_path, char* err, size_t errlen) {
  const int rc = guarded([&] {
    if (!conf_json_path) throw std::runtime_error("config path is NULL");
    const std::string path(conf_json_path);
    const std::string text = read_file(path);
    json::Value v = json::parse(text.c_str());
    auto conf = std::make_shared<Config>();
    MatchOptions base = default_options();
    const json::Value* meili = v.get("meili");
    if (meili) apply_options(meili->get("default"), base);
    for (int m = 0; m < 5; ++m) {
      conf->mode_defaults[m] = base;
      conf->mode_defaults[m].mode = m;
      if (meili) apply_options(meili->get(kModeNames[m]), conf->mode_defaults[m]);
    }
    // meili's turn costs (DESIGN.md §3 rule 3b): the stock valhalla_build_config sets 200 / 140 /
    // 100 for auto / bicycle / pedestrian, and the engine applies them.  reporter_amd.ignore_turn_penalty
    // (an explicit opt-out, e.g. to compare with a zero-turn-cost deployment) matches without them.
    bool ignore_turn = false;
    if (const json::Value* ra = v.get("reporter_amd"))
      if (const json::Value* it = ra->get("ignore_turn_penalty"); it && it->type == json::Value::Bool) ignore_turn = it->b;
    for (int m = 0; m < 5; ++m) {
      if (!turn_factor_ok(conf->mode_defaults[m].turn_penalty_factor))
        throw std::runtime_error(std::string("meili ") + kModeNames[m] + ": " + kTurnPenaltyError);
      if (ignore_turn) conf->mode_defaults[m].turn_penalty_factor = 0.f;
    }
    std::string graph;
    int device = g_device;
    if (const json::Value* ra = v.get("reporter_amd")) {
      if (const json::Value* gp = ra->get("graph"); gp && gp->type == json::Value::String) graph = gp->str;
      if (const json::Value* dv = ra->get("device"); dv && dv->is_num()) device = (int)dv->num;
    }
    if (graph.empty()) {
      if (const json::Value* mj = v.get("mjolnir"))
        if (const json::Value* te = mj->get("tile_extract"); te && te->type == json::Value::String) graph = te->str;
    }
    if (graph.empty()) throw std::runtime_error("config names no graph (reporter_amd.graph or mjolnir.tile_extract)");
    if (graph[0] != '/') graph = dir_of(path) + "/" + graph;
    bool coalesce = true;
    double window_ms = 0.0;
    size_t max_traces = 16384;
    // reporter_amd.coalesce_workers: dispatcher threads, each a matcher on its own stream, so one
    // batch's latency-bound kernels overlap the next batch's (C-ABI client, 64 clients of 600-point
    // requests: 1 -> 2 workers 23 -> 30 M points/s; round 3's Python clients saw no gain)
    int workers = 2;
    double ball_radius_m = -1.0;   // < 0: engine default (automatic from the graph's density, or RM_BALL_RADIUS_M)
    if (const json::Value* ra = v.get("reporter_amd")) {
      if (const json::Value* br = ra->get("ball_radius"); br && br->is_num()) {
        ball_radius_m = br->num;
        if (!(ball_radius_m >= 0.0) || ball_radius_m * 100.0 > kBallMaxRadiusCm)
          throw std::runtime_error("reporter_amd.ball_radius out of range (0..10000 m)");
      }
      if (const json::Value* c = ra->get("coalesce"); c && c->type == json::Value::Bool) coalesce = c->b;
      if (const json::Value* w = ra->get("coalesce_window_ms"); w && w->is_num()) window_ms = w->num;
      if (const json::Value* mx = ra->get("coalesce_max_traces"); mx && mx->is_num()) max_traces = (size_t)mx->num;
      if (const json::Value* wk = ra->get("coalesce_workers"); wk && wk->is_num()) workers = (int)wk->num;
    }
    // travel modes whose route tables are built now, so no request waits for a build (the Java
    // caller gives up after 10 s, HttpClient.java:80-87): auto (the default mode) and the modes
    // reporter_amd.modes lists.  Other modes build on their first request (time
    // and HBM per mode).  The stock meili config has auto / bicycle / pedestrian sections, so
    // building every mode with a section would cost up to half the HBM at startup for modes a
    // deployment may never see.
    uint32_t modes = 1u << kModeAuto;
    if (const json::Value* ra = v.get("reporter_amd")) {
      if (const json::Value* ml = ra->get("modes")) {
        if (ml->type != json::Value::Array) throw std::runtime_error("reporter_amd.modes must be a list of mode names");
        for (const json::Value& x : ml->arr) {
          if (x.type != json::Value::String) throw std::runtime_error("reporter_amd.modes must be a list of mode names");
          modes |= 1u << mode_from_name(x.str);
        }
      }
    }
    Graph g = Graph::load(graph);
    conf->engine = std::make_shared<Engine>(g, device);
    if (ball_radius_m >= 0.0) conf->engine->set_ball_radius((uint32_t)(ball_radius_m * 100.0));
    conf->engine->ensure_balls(modes);
    // and the turn rows of those whose configured turn_penalty_factor is > 0 (rule 3b), so the
    // first request with turn costs does not build them either
    uint32_t turn_modes = 0;
    for (int m = 0; m < 5; ++m)
      if (((modes >> m) & 1u) && conf->mode_defaults[m].turn_penalty_factor > 0.f) turn_modes |= 1u << m;
    if (turn_modes) conf->engine->ensure_turn_rows(turn_modes);
    if (coalesce) conf->coalescer = std::make_unique<Coalescer>(conf->engine, window_ms, max_traces, workers);
    std::lock_guard<std::mutex> lk(g_mu);
    g_conf = conf;
  });
  if (rc && err && errlen) {
    std::strncpy(err, g_err.c_str(), errlen - 1);
    err[errlen - 1] = 0;
  }
  return rc;
}

rm_matcher* rm_matcher_create(void) {
  rm_matcher* out = nullptr;
  guarded([&] {
    std::shared_ptr<Config> c;
    {
      std::lock_guard<std::mutex> lk(g_mu);
      c = g_conf;
    }
    if (!c) throw std::runtime_error("valhalla.Configure has not been called");
    auto m = std::make_unique<rm_matcher>();
    m->conf = c;
    if (!c->coalescer) m->m = std::make_unique<Matcher>(c->engine.get());   // else created on first batch call
    out = m.release();
  });
  return out;
}

void rm_matcher_destroy(rm_matcher* m) { delete m; }

int rm_match_batch(rm_matcher* m, const char* const* traces, size_t n, char** outs) {
  return guarded([&] {
    if (!m) throw std::runtime_error("matcher is NULL");
    for (size_t i = 0; i < n; ++i) outs[i] = nullptr;
    if (n == 0) return;
    for (size_t i = 0; i < n; ++i)
      if (!traces[i]) throw std::runtime_error("trace string is NULL");
    if (n == 1 && m->conf->coalescer) {
      ParsedTrace pt = parse_trace(traces[0], *m->conf);
      const std::string js = m->conf->coalescer->submit(&pt, &m->m);
      outs[0] = dup_string(js);
      return;
    }
    try {
      match_json_batch(m, traces, n, outs);   // any failing trace fails the call, naming the trace
    } catch (...) {
      for (size_t i = 0; i < n; ++i) { std::free(outs[i]); outs[i] = nullptr; }
      throw;
    }
  });
}

int rm_match_batch_packed(rm_matcher* m, const char* const* traces, size_t n, char** buf, uint64_t* off) {
  return guarded([&] {
    if (!m) throw std::runtime_error("matcher is NULL");
    if (!buf || !off) throw std::runtime_error("buf / off is NULL");
    *buf = nullptr;
    off[0] = 0;
    for (size_t i = 0; i < n; ++i)
      if (!traces[i]) throw std::runtime_error("trace string is NULL");
    if (n == 0) {
      *buf = static_cast<char*>(std::calloc(1, 1));
      return;
    }
    if (n == 1 && m->conf->coalescer) {   // one request: the coalescer, as rm_match
      ParsedTrace pt = parse_trace(traces[0], *m->conf);
      const std::string js = m->conf->coalescer->submit(&pt, &m->m);
      char* b = static_cast<char*>(std::malloc(js.size() + 1));
      if (!b) throw std::bad_alloc();
      std::memcpy(b, js.data(), js.size());
      b[js.size()] = 0;
      off[1] = js.size();
      *buf = b;
      return;
    }
    const PackedOut pk{buf, off};
    match_json_batch(m, traces, n, nullptr, &pk);   // any failing trace fails the call, naming the trace
  });
}

int rm_match_points_batch(rm_matcher* m, const char* const* traces, size_t n, char** outs) {
  return guarded([&] {
    if (!m) throw std::runtime_error("matcher is NULL");
    for (size_t i = 0; i < n; ++i) outs[i] = nullptr;
    if (n == 0) return;
    for (size_t i = 0; i < n; ++i)
      if (!traces[i]) throw std::runtime_error("trace string is NULL");
    try {
      match_json_batch(m, traces, n, outs, nullptr, true);   // uncoalesced, whatever n is
    } catch (...) {
      for (size_t i = 0; i < n; ++i) { std::free(outs[i]); outs[i] = nullptr; }
      throw;
    }
  });
}

int rm_match_points(rm_matcher* m, const char* trace_json, char** out_json) {
  if (!out_json) return fail("out_json is NULL");
  *out_json = nullptr;
  return rm_match_points_batch(m, &trace_json, 1, out_json);
}

int rm_match_edges_batch(rm_matcher* m, const char* const* traces, size_t n, char** outs) {
  return guarded([&] {
    if (!m) throw std::runtime_error("matcher is NULL");
    for (size_t i = 0; i < n; ++i) outs[i] = nullptr;
    if (n == 0) return;
    for (size_t i = 0; i < n; ++i)
      if (!traces[i]) throw std::runtime_error("trace string is NULL");
    try {
      match_json_batch(m, traces, n, outs, nullptr, false, true);   // uncoalesced, whatever n is
    } catch (...) {
      for (size_t i = 0; i < n; ++i) { std::free(outs[i]); outs[i] = nullptr; }
      throw;
    }
  });
}

int rm_match_edges(rm_matcher* m, const char* trace_json, char** out_json) {
  if (!out_json) return fail("out_json is NULL");
  *out_json = nullptr;
  return rm_match_edges_batch(m, &trace_json, 1, out_json);
}

int rm_report_batch(rm_matcher* m, const char* const* traces, size_t n, double threshold_sec, char** outs) {
  return guarded([&] {
    if (!m) throw std::runtime_error("matcher is NULL");
    for (size_t i = 0; i < n; ++i) outs[i] = nullptr;
    check_threshold(threshold_sec);
    if (n == 0) return;
    for (size_t i = 0; i < n; ++i)
      if (!traces[i]) throw std::runtime_error("trace string is NULL");
    ReportCall rc;
    rc.threshold = threshold_sec;
    try {
      match_json_batch(m, traces, n, outs, nullptr, false, false, &rc);   // any failing trace fails the call, naming the trace
    } catch (...) {
      for (size_t i = 0; i < n; ++i) { std::free(outs[i]); outs[i] = nullptr; }
      throw;
    }
  });
}

int rm_report_batch_packed(rm_matcher* m, const char* const* traces, size_t n, double threshold_sec, char** buf,
                           uint64_t* off) {
  return guarded([&] {
    if (!m) throw std::runtime_error("matcher is NULL");
    if (!buf || !off) throw std::runtime_error("buf / off is NULL");
    *buf = nullptr;
    off[0] = 0;
    check_threshold(threshold_sec);
    for (size_t i = 0; i < n; ++i)
      if (!traces[i]) throw std::runtime_error("trace string is NULL");
    if (n == 0) {
      *buf = static_cast<char*>(std::calloc(1, 1));
      return;
    }
    ReportCall rc;
    rc.threshold = threshold_sec;
    const PackedOut pk{buf, off};
    match_json_batch(m, traces, n, nullptr, &pk, false, false, &rc);
  });
}

int rm_report(rm_matcher* m, const char* trace_json, double threshold_sec, char** out_json) {
  if (!out_json) return fail("out_json is NULL");
  *out_json = nullptr;
  return guarded([&] {
    if (!m) throw std::runtime_error("matcher is NULL");
    if (!trace_json) throw std::runtime_error("trace string is NULL");
    check_threshold(threshold_sec);
    if (!m->conf->coalescer) {
      ReportCall rc;
      rc.threshold = threshold_sec;
      match_json_batch(m, &trace_json, 1, out_json, nullptr, false, false, &rc);
      return;
    }
    ParsedTrace pt = parse_report_trace(trace_json, *m->conf, threshold_sec);
    const std::string js = m->conf->coalescer->submit(&pt, &m->m);
    *out_json = dup_string(js);
  });
}

int rm_report_info(const rm_matcher* m, uint64_t out[4]) {
  return guarded([&] {
    if (!m || !out) throw std::runtime_error("matcher or out is NULL");
    for (int i = 0; i < 4; ++i) out[i] = m->reply_info[i];
  });
}

int rm_match(rm_matcher* m, const char* trace_json, char** out_json) {
  if (!out_json) return fail("out_json is NULL");
  *out_json = nullptr;
  return rm_match_batch(m, &trace_json, 1, out_json);
}

void rm_free(char* p) { std::free(p); }

int rm_matcher_timing(const rm_matcher* m, double out[6]) {
  return guarded([&] {
    if (!m || !out) throw std::runtime_error("matcher or out is NULL");
    for (int i = 0; i < 6; ++i) out[i] = m->ms[i];
  });
}

int rm_coalesce_timing(double out[4]) {
  return guarded([&] {
    std::shared_ptr<Config> c;
    {
      std::lock_guard<std::mutex> lk(g_mu);
      c = g_conf;
    }
    for (int i = 0; i < 4; ++i) out[i] = 0.0;
    if (c && c->coalescer) c->coalescer->timing(out);
  });
}

int rm_coalesce_stats(uint64_t out[4]) {
  return guarded([&] {
    std::shared_ptr<Config> c;
    {
      std::lock_guard<std::mutex> lk(g_mu);
      c = g_conf;
    }
    for (int i = 0; i < 4; ++i) out[i] = 0;
    if (c && c->coalescer) c->coalescer->stats(out);
  });
}

// ---------------- world ----------------
void rm_default_world_params(rm_world_params* p) {
  WorldParams d;
  p->rows = d.rows; p->cols = d.cols; p->block_m = d.block_m; p->seed = d.seed;
  p->center_lat = d.center_lat; p->center_lon = d.center_lon; p->jitter = d.jitter;
  p->arterial_every = d.arterial_every; p->highway_every = d.highway_every;
  p->segment_max_m = d.segment_max_m; p->internal_m = d.internal_m; p->service_frac = d.service_frac;
  p->oneway_frac = d.oneway_frac; p->curve_frac = d.curve_frac; p->cell_m = d.cell_m;
}

int rm_world_build(const rm_world_params* p, const char* out_path) {
  return guarded([&] {
    WorldParams w;
    w.rows = p->rows; w.cols = p->cols; w.block_m = p->block_m; w.seed = p->seed;
    w.center_lat = p->center_lat; w.center_lon = p->center_lon; w.jitter = p->jitter;
    w.arterial_every = p->arterial_every; w.highway_every = p->highway_every;
    w.segment_max_m = p->segment_max_m; w.internal_m = p->internal_m; w.service_frac = p->service_frac;
    w.oneway_frac = p->oneway_frac; w.curve_frac = p->curve_frac; w.cell_m = p->cell_m;
    build_world(w).save(out_path);
  });
}

int rm_graph_info(const char* graph_path, uint64_t out[7]) {
  return guarded([&] {
    Graph g = Graph::load(graph_path);
    out[0] = g.num_nodes(); out[1] = g.num_edges(); out[2] = g.num_roads(); out[3] = g.num_verts();
    out[4] = g.num_segments(); out[5] = (uint64_t)g.grid.ncx * g.grid.ncy; out[6] = g.grid.cell_item.size();
  });
}

int rm_graph_export_osm(const char* graph_path, const char* osm_path) {
  return guarded([&] {
    if (!graph_path || !osm_path) throw std::runtime_error("path is NULL");
    export_osm(Graph::load(graph_path), osm_path);
  });
}

int rm_graph_export_pbf(const char* graph_path, const char* pbf_path) {
  return guarded([&] {
    if (!graph_path || !pbf_path) throw std::runtime_error("path is NULL");
    export_osm_pbf(Graph::load(graph_path), pbf_path);
  });
}

int rm_graph_import_osm(const char* osm_path, const char* graph_path, double cell_m) {
  return guarded([&] {
    if (!graph_path || !osm_path) throw std::runtime_error("path is NULL");
    import_osm(osm_path, cell_m).save(graph_path);
  });
}

void rm_default_city_params(rm_city_params* p) {
  const CityParams d;
  p->rows = d.rows; p->cols = d.cols; p->block_m = d.block_m; p->seed = d.seed;
  p->center_lat = d.center_lat; p->center_lon = d.center_lon; p->jitter = d.jitter;
  p->primary_every = d.primary_every; p->secondary_every = d.secondary_every;
  p->boulevard_every = d.boulevard_every; p->diagonal_every = d.diagonal_every;
  p->roundabout_frac = d.roundabout_frac; p->drop_frac = d.drop_frac; p->oneway_frac = d.oneway_frac;
  p->spur_frac = d.spur_frac; p->service_frac = d.service_frac; p->footway_frac = d.footway_frac;
  p->osmlr_local_frac = d.osmlr_local_frac; p->way_max_m = d.way_max_m; p->trunk = d.trunk;
}

int rm_osm_city_write(const rm_city_params* p, const char* osm_path, int pbf) {
  return guarded([&] {
    if (!p || !osm_path) throw std::runtime_error("params or path is NULL");
    CityParams c;
    c.rows = p->rows; c.cols = p->cols; c.block_m = p->block_m; c.seed = p->seed;
    c.center_lat = p->center_lat; c.center_lon = p->center_lon; c.jitter = p->jitter;
    c.primary_every = p->primary_every; c.secondary_every = p->secondary_every;
    c.boulevard_every = p->boulevard_every; c.diagonal_every = p->diagonal_every;
    c.roundabout_frac = p->roundabout_frac; c.drop_frac = p->drop_frac; c.oneway_frac = p->oneway_frac;
    c.spur_frac = p->spur_frac; c.service_frac = p->service_frac; c.footway_frac = p->footway_frac;
    c.osmlr_local_frac = p->osmlr_local_frac; c.way_max_m = p->way_max_m; c.trunk = p->trunk;
    std::unique_ptr<OsmSink> sink = pbf ? make_osm_pbf_sink(osm_path) : make_osm_xml_sink(osm_path);
    write_osm_city(c, *sink);
  });
}

void rm_default_trace_params(rm_trace_params* p) {
  TraceParams d;
  p->n_traces = d.n_traces; p->n_points = d.n_points; p->rate_s = d.rate_s; p->noise_m = d.noise_m;
  p->seed = d.seed; p->mode = d.mode; p->start_epoch = d.start_epoch; p->threads = d.threads;
}

int rm_traces_generate(const char* graph_path, const rm_trace_params* p, double* lon, double* lat, double* time,
                       float* accuracy, uint32_t* truth_edge, uint32_t* truth_off_cm) {
  return rm_traces_generate_ids(graph_path, p, nullptr, lon, lat, time, accuracy, truth_edge, truth_off_cm);
}

int rm_traces_generate_ids(const char* graph_path, const rm_trace_params* p, const uint32_t* ids, double* lon,
                           double* lat, double* time, float* accuracy, uint32_t* truth_edge, uint32_t* truth_off_cm) {
  return guarded([&] {
    Graph g = Graph::load(graph_path);
    TraceParams t;
    t.n_traces = p->n_traces; t.n_points = p->n_points; t.rate_s = p->rate_s; t.noise_m = p->noise_m;
    t.seed = p->seed; t.mode = p->mode; t.start_epoch = p->start_epoch; t.threads = p->threads;
    TraceSet ts = generate_traces(g, t, ids);
    const size_t P = ts.lon.size();
    std::memcpy(lon, ts.lon.data(), P * 8); std::memcpy(lat, ts.lat.data(), P * 8);
    std::memcpy(time, ts.time.data(), P * 8); std::memcpy(accuracy, ts.accuracy.data(), P * 4);
    if (truth_edge) std::memcpy(truth_edge, ts.truth_edge.data(), P * 4);
    if (truth_off_cm) std::memcpy(truth_off_cm, ts.truth_off_cm.data(), P * 4);
  });
}

// ---------------- engine / runner ----------------
rm_engine* rm_engine_create(const char* graph_path, int device) {
  rm_engine* out = nullptr;
  guarded([&] {
    Graph g = Graph::load(graph_path);
    auto e = std::make_unique<rm_engine>();
    e->e = std::make_shared<Engine>(g, device);
    out = e.release();
  });
  return out;
}
void rm_engine_destroy(rm_engine* e) { delete e; }
uint32_t rm_engine_n_segments(const rm_engine* e) { return e ? e->e->n_segments() : 0; }
int rm_engine_segment_ids(const rm_engine* e, uint64_t* ids) {
  return guarded([&] {
    const auto& v = e->e->host().seg_id;
    std::memcpy(ids, v.data(), v.size() * 8);
  });
}

int rm_engine_set_ball_radius(rm_engine* e, double radius_m) {
  return guarded([&] {
    if (!(radius_m >= 0.0) || radius_m * 100.0 > kBallMaxRadiusCm) throw std::runtime_error("ball radius out of range (0..10000 m)");
    e->e->set_ball_radius((uint32_t)(radius_m * 100.0));
  });
}
int rm_engine_ball_stats(const rm_engine* e, int mode, double out[6]) {
  return guarded([&] {
    if (mode < 0 || mode > kModePedestrian) throw std::runtime_error("unknown travel mode");
    out[0] = e->e->mode_ball_radius(mode) / 100.0;
    e->e->ball_stats(mode, out + 1);
    out[5] = ((e->e->ball_gpu_mask() >> mode) & 1u) ? 1.0 : 0.0;
  });
}

int rm_engine_turn_rows(const rm_engine* e, uint32_t* mode_mask, double* build_ms) {
  return guarded([&] {
    *mode_mask = e->e->turn_row_mask();
    for (int m = 0; m < 5; ++m) build_ms[m] = e->e->turn_build_ms(m);
  });
}
int rm_engine_grid_alt(const rm_engine* e, uint32_t* f, float* radius_m) {
  return guarded([&] {
    *f = e->e->grid_alt_split();
    *radius_m = e->e->grid_alt_radius();
  });
}

int rm_engine_grid_split(const rm_engine* e, uint32_t* f) {
  return guarded([&] { *f = e->e->grid_split(); });
}

int rm_engine_ball_lookup(rm_engine* e, int mode, uint64_t n, const uint32_t* from, const uint32_t* road,
                          uint64_t* keys, uint8_t* preds) {
  return guarded([&] {
    if (!e) throw std::runtime_error("engine is NULL");
    if (mode < 0 || mode > kModePedestrian) throw std::runtime_error("unknown travel mode");
    e->e->ball_lookup(mode, n, from, road, keys, preds);
  });
}

int rm_graph_grid_split(const char* graph_path, uint32_t* f) {
  return guarded([&] {
    if (!f) throw std::runtime_error("f is NULL");
    *f = choose_grid_split(Graph::load(graph_path));
  });
}

int rm_graph_auto_ball_radius(const char* graph_path, double* radius_m) {
  return guarded([&] {
    if (!radius_m) throw std::runtime_error("radius_m is NULL");
    *radius_m = auto_ball_radius_cm(Graph::load(graph_path)) / 100.0;
  });
}

int rm_graph_fit_ball_radius(const char* graph_path, int mode, double start_m, double avail_gb, double* radius_m) {
  return guarded([&] {
    if (!graph_path || !radius_m) throw std::runtime_error("path or radius_m is NULL");
    if (mode < 0 || mode > kModePedestrian) throw std::runtime_error("unknown travel mode");
    if (!(start_m >= 0.0) || start_m * 100.0 > kBallMaxRadiusCm) throw std::runtime_error("ball radius out of range (0..10000 m)");
    if (!(avail_gb >= 0.0)) throw std::runtime_error("avail_gb must be non-negative");
    const uint64_t avail = (uint64_t)std::min(avail_gb * (double)(1ull << 30), 1.8e19);
    *radius_m = fit_ball_radius_cm(Graph::load(graph_path), mode, (uint32_t)(start_m * 100.0), avail) / 100.0;
  });
}

int rm_graph_ball_sample(const char* graph_path, int mode, double radius_m, double out[3]) {
  return guarded([&] {
    if (!graph_path || !out) throw std::runtime_error("path or out is NULL");
    if (mode < 0 || mode > kModePedestrian) throw std::runtime_error("unknown travel mode");
    if (!(radius_m >= 0.0) || radius_m * 100.0 > kBallMaxRadiusCm) throw std::runtime_error("ball radius out of range (0..10000 m)");
    const BallSample bs = sample_balls(Graph::load(graph_path), (uint32_t)(radius_m * 100.0), kBallMaxKeysHost, mode);
    out[0] = bs.nodes; out[1] = bs.table_bytes; out[2] = bs.skipped_frac;
  });
}

int rm_balls_lookup(const char* graph_path, int mode, double radius_m, uint64_t n, const uint32_t* from,
                    const uint32_t* road, uint64_t* keys, uint8_t* preds) {
  return guarded([&] {
    if (mode < 0 || mode > kModePedestrian) throw std::runtime_error("unknown travel mode");
    if (!(radius_m >= 0.0) || radius_m * 100.0 > kBallMaxRadiusCm) throw std::runtime_error("ball radius out of range (0..10000 m)");
    Graph g = Graph::load(graph_path);
    BallTables bt;
    build_balls(g, mode, (uint32_t)(radius_m * 100.0), kBallMaxKeysHost, 4, bt);
    for (uint64_t i = 0; i < n; ++i) {
      keys[2 * i] = keys[2 * i + 1] = kKeyInf;
      if (preds) preds[2 * i] = preds[2 * i + 1] = (uint8_t)kBallPredNone;
      if (from[i] >= g.num_nodes() || road[i] >= g.num_roads()) throw std::runtime_error("node or road out of range");
      const uint32_t off = bt.hdr[2 * (size_t)from[i]], bits = bt.hdr[2 * (size_t)from[i] + 1];
      if (!bits) continue;
      const uint32_t mask = (1u << bits) - 1u;
      for (uint32_t s = ball_slot(road[i], bits);; s = (s + 1) & mask) {
        const uint32_t* e = bt.ent.data() + 4 * (ball_row0(off) + s);
        if (e[0] == kNone) break;
        if ((e[0] & bt.road_mask) != road[i]) continue;
        keys[2 * i] = ball_key0(e[0], e[1], e[3]);
        keys[2 * i + 1] = ball_key1(e[0], e[2], e[3]);
        if (preds) {
          preds[2 * i] = (uint8_t)ball_pred(e[0], 0, bt.road_mask);
          preds[2 * i + 1] = (uint8_t)ball_pred(e[0], 1, bt.road_mask);
        }
        break;
      }
    }
  });
}

rm_runner* rm_runner_create(rm_engine* e) {
  rm_runner* out = nullptr;
  guarded([&] {
    if (!e) throw std::runtime_error("engine is NULL");
    auto r = std::make_unique<rm_runner>();
    r->e = e->e;
    r->m = std::make_unique<Matcher>(e->e.get());
    out = r.release();
  });
  return out;
}
void rm_runner_destroy(rm_runner* r) { delete r; }

void rm_default_run_params(rm_run_params* p) {
  p->threshold_sec = 15.0; p->report_mask = 0x6; p->transition_mask = 0x6; p->hist_dev = nullptr; p->do_report = 1;
  p->zero_hist = 0; p->dur_dev = nullptr;
}

static RunParams to_rp(const rm_run_params* p) {
  RunParams rp;
  if (p) {
    rp.threshold_sec = p->threshold_sec; rp.report_mask = p->report_mask; rp.transition_mask = p->transition_mask;
    rp.hist = p->hist_dev; rp.do_report = p->do_report; rp.zero_hist = p->zero_hist;
    rp.dur = (unsigned long long*)p->dur_dev;
  }
  return rp;
}

int rm_runner_run(rm_runner* r, const rm_batch_desc* b, const rm_run_params* p) {
  return guarded([&] {
    HostBatch hb;
    hb.n_traces = b->n_traces; hb.trace_off = b->trace_off; hb.lon = b->lon; hb.lat = b->lat; hb.time = b->time;
    hb.accuracy = b->accuracy; hb.n_opts = b->n_opts; hb.opts = (const MatchOptions*)b->opts; hb.trace_opt = b->trace_opt;
    r->m->run(hb, to_rp(p));
  });
}
int rm_runner_rerun(rm_runner* r, const rm_run_params* p) { return guarded([&] { r->m->run_device(to_rp(p)); }); }

int rm_runners_rerun(rm_runner* const* rs, uint32_t n, const rm_run_params* p) {
  return guarded([&] {
    if (!rs || n == 0) throw std::runtime_error("no runners");
    for (uint32_t i = 0; i < n; ++i)
      if (!rs[i]) throw std::runtime_error("runner is NULL");
    RunParams rp = to_rp(p);
    if ((rp.hist || rp.dur) && rp.zero_hist && rp.do_report) {
      // the parts add into one histogram: zero it once before any part reports
      hipStream_t st = rs[0]->m->stream();
      const size_t nseg = rs[0]->m->engine().n_segments();
      if (rp.hist) RM_HIP(hipMemsetAsync(rp.hist, 0, nseg * kHistBins * sizeof(uint32_t), st));
      if (rp.dur) RM_HIP(hipMemsetAsync(rp.dur, 0, nseg * 8u, st));
      RM_HIP(hipStreamSynchronize(st));
    }
    rp.zero_hist = false;
    // one host thread per part: each part's read-backs block only its own thread, so the parts'
    // kernels run concurrently on their streams
    std::vector<std::exception_ptr> err(n);
    std::vector<std::thread> th;
    th.reserve(n - 1);
    for (uint32_t i = 1; i < n; ++i)
      th.emplace_back([&, i] {
        try { rs[i]->m->run_device(rp); } catch (...) { err[i] = std::current_exception(); }
      });
    try { rs[0]->m->run_device(rp); } catch (...) { err[0] = std::current_exception(); }
    for (auto& t : th) t.join();
    for (auto& e : err)
      if (e) std::rethrow_exception(e);
  });
}
int rm_runner_sizes(rm_runner* r, uint64_t out[10]) {
  return guarded([&] {
    out[0] = r->m->n_points(); out[1] = r->m->n_traces(); out[2] = r->m->n_trans(); out[3] = r->m->n_path_edges();
    out[4] = r->m->count_segments(); out[5] = r->m->count_reports();
    uint32_t t[4];
    r->m->tier_counts(t);
    for (int i = 0; i < 4; ++i) out[6 + i] = t[i];
  });
}
int rm_runner_route_tiers(rm_runner* r, uint64_t out[10]) {
  return guarded([&] {
    uint32_t c[kCtlWords];
    r->m->ctl_words(c);
    out[0] = c[kCtlBallToSearch]; out[1] = c[kCtlLaneToReg2]; out[2] = c[kCtlReg2ToGroup];
    out[3] = c[kCtlPathsBallToSearch]; out[4] = c[kCtlWaveToGlobal]; out[5] = c[kCtlPathsWaveToGlobal];
    out[6] = c[kCtlGroupToWave512]; out[7] = c[kCtlPathsGroupToWave512];
    out[8] = c[kCtlWave512ToWave4096]; out[9] = c[kCtlPathsWave512ToWave4096];
  });
}
int rm_runner_run_stats(rm_runner* r, uint64_t out[4]) { return guarded([&] { r->m->run_stats(out); }); }
int rm_scan_block_bases(const uint64_t* part, uint32_t nb, uint32_t lanes, uint64_t* base) {
  return guarded([&] {
    if (!lanes) throw std::invalid_argument("lanes must be positive");
    std::vector<unsigned long long> p(2 * (size_t)nb), bkt(2 * (size_t)scan_buckets(nb) + 2, 0ull);
    for (size_t i = 0; i < p.size(); ++i) p[i] = part[i];
    for (uint32_t q = 0; q < nb; ++q) {   // as k_scan_buckets does
      bkt[2 * (size_t)scan_bucket(q)] += p[2 * (size_t)q];
      bkt[2 * (size_t)scan_bucket(q) + 1] += p[2 * (size_t)q + 1];
    }
    for (uint32_t q = 0; q < nb; ++q) {   // as an apply block does, lane by lane
      unsigned long long a = 0, c = 0;
      for (uint32_t l = 0; l < lanes; ++l) {
        unsigned long long la, lc;
        scan_base_lane(p.data(), bkt.data(), q, l, lanes, la, lc);
        a += la; c += lc;
      }
      base[2 * (size_t)q] = a; base[2 * (size_t)q + 1] = c;
    }
  });
}
int rm_runner_get_states(rm_runner* r, uint32_t* a, uint32_t* b) { return guarded([&] { r->m->get_states(a, b); }); }
int rm_runner_get_candidates(rm_runner* r, uint8_t* a, uint32_t* b, uint32_t* c, float* d) {
  return guarded([&] { r->m->get_candidates(a, b, c, d); });
}
int rm_runner_get_routes(rm_runner* r, uint32_t* a, double* b, uint32_t* c) { return guarded([&] { r->m->get_routes(a, b, c); }); }
int rm_runner_get_route_terms(rm_runner* r, double* a, int* present) {
  return guarded([&] { *present = r->m->get_route_terms(a); });
}
int rm_runner_get_viterbi(rm_runner* r, int8_t* a, uint8_t* b) { return guarded([&] { r->m->get_viterbi(a, b); }); }
int rm_runner_get_paths(rm_runner* r, uint32_t* a, uint32_t* b, uint32_t* c, uint32_t* d) {
  return guarded([&] { r->m->get_paths(a, b, c, d); });
}
int rm_runner_get_matched_points(rm_runner* r, rm_matched_point* out) {
  static_assert(sizeof(rm_matched_point) == sizeof(MatchedPoint), "rm_matched_point is rm::MatchedPoint");
  return guarded([&] { r->m->matched_points(reinterpret_cast<MatchedPoint*>(out)); });
}
int rm_runner_matched_edges(rm_runner* r, uint64_t out[2]) {
  return guarded([&] { r->m->matched_edges(out); });
}
int rm_runner_get_matched_edges(rm_runner* r, uint32_t* edge_off, rm_matched_edge* edges, uint32_t* shape_off, float* shape) {
  static_assert(sizeof(rm_matched_edge) == sizeof(MatchedEdge), "rm_matched_edge is rm::MatchedEdge");
  return guarded([&] { r->m->get_matched_edges(edge_off, reinterpret_cast<MatchedEdge*>(edges), shape_off, shape); });
}
int rm_runner_matched_edges_time(rm_runner* r, double* ms) {
  return guarded([&] { *ms = r->m->matched_edges_ms(); });
}
int rm_runner_get_segments(rm_runner* r, uint32_t* off, void* segs) {
  return guarded([&] { r->m->get_segments(off, (SegmentRec*)segs); });
}
int rm_runner_get_reports(rm_runner* r, uint32_t* off, void* reps, void* stats) {
  return guarded([&] { r->m->get_reports(off, (ReportRec*)reps, (ReportStats*)stats); });
}
int rm_runner_set_timing(rm_runner* r, int on) { return guarded([&] { r->m->set_timing(on != 0); }); }
int rm_runner_set_timing_mask(rm_runner* r, uint32_t mask) { return guarded([&] { r->m->set_timing_mask(mask); }); }
int rm_runner_set_isolation(rm_runner* r, int on) { return guarded([&] { r->m->set_isolation(on != 0); }); }
int rm_runner_set_locality(rm_runner* r, int mode) {
  return guarded([&] {
    if (mode < -1 || mode > 2) throw std::runtime_error("locality mode must be -1, 0, 1 or 2");
    r->m->set_locality(mode);
  });
}
int rm_runner_locality_used(rm_runner* r, int* used) { return guarded([&] { *used = r->m->locality_used() ? 1 : 0; }); }
int rm_runner_trace_errors(rm_runner* r, uint32_t* errs) { return guarded([&] { r->m->get_trace_errors(errs); }); }
int rm_report_segments(const rm_report_desc* d, uint32_t* rep_off, void* reps, void* stats) {
  return guarded([&] {
    if (!d || !rep_off || (d->n_traces && (!d->seg_off || !d->trace_end_time || !d->threshold_sec || !d->report_mask ||
                                           !d->transition_mask || !stats)))
      throw std::runtime_error("report descriptor or output is NULL");
    report_segments(g_device, d->n_traces, d->seg_off, (const SegmentRec*)d->segs, d->trace_end_time, d->threshold_sec,
                    d->report_mask, d->transition_mask, rep_off, (ReportRec*)reps, (ReportStats*)stats);
  });
}
int rm_report_replies(const rm_report_desc* d, int writer, char** buf, uint64_t* off, uint64_t info[4]) {
  return guarded([&] {
    if (!d || !buf || !off || (d->n_traces && (!d->seg_off || !d->trace_end_time || !d->threshold_sec || !d->report_mask ||
                                               !d->transition_mask)))
      throw std::runtime_error("report descriptor or output is NULL");
    if (writer < 0 || writer > 2) throw std::runtime_error("reply writer must be 0, 1 or 2");
    const uint32_t T = d->n_traces;
    const uint64_t S = T ? d->seg_off[T] : 0;
    // by size: the segments stand in for the points a matcher run is judged by
    const int used = writer ? writer : (S > reply_device_min_points() ? 2 : 1);
    uint64_t flagged = 0;
    double ms = 0.0;
    const SegmentRec* segs = (const SegmentRec*)d->segs;
    if (used == 2) {
      DeviceReports dr;
      if (T) report_segments_device(g_device, T, d->seg_off, segs, d->trace_end_time, d->threshold_sec, d->report_mask,
                                    d->transition_mask, dr);
      ReplySource src;
      src.T = T; src.seg_base = dr.seg_off; src.seg_cnt = dr.seg_cnt; src.rep_base = dr.seg_off;
      src.segs = dr.segs; src.reps = dr.reps; src.stats = dr.stats; src.cap = S;
      ReplyWriter w;
      w.write(g_device, nullptr, src, buf, off, &flagged, &ms);
    } else {
      std::vector<uint32_t> rep_off(T + 1, 0u);
      std::vector<ReportRec> reps(std::max<uint64_t>(S, 1));
      std::vector<ReportStats> stats(std::max<uint32_t>(T, 1));
      report_segments(g_device, T, d->seg_off, segs, d->trace_end_time, d->threshold_sec, d->report_mask, d->transition_mask,
                      rep_off.data(), reps.data(), stats.data());
      std::vector<uint32_t> rep_cnt(T);
      for (uint32_t k = 0; k < T; ++k) rep_cnt[k] = rep_off[k + 1] - rep_off[k];
      const uint32_t zero[1] = {0u};
      reply_format_host(T, T ? d->seg_off : zero, segs, rep_off.data(), rep_cnt.data(), reps.data(), stats.data(), buf, off, &flagged);
    }
    if (info) { info[0] = off[T]; info[1] = flagged; info[2] = (uint64_t)used; info[3] = (uint64_t)(ms * 1000.0 + 0.5); }
  });
}
int rm_report_format_host(uint32_t n, const uint32_t* seg_off, const void* segs, const uint32_t* rep_off, const void* reps,
                          const void* stats, char** buf, uint64_t* off) {
  return guarded([&] {
    if (!buf || !off || (n && (!seg_off || !rep_off || !stats))) throw std::runtime_error("reply records or output is NULL");
    const uint32_t zero[1] = {0u};
    std::vector<uint32_t> rep_cnt(n);
    for (uint32_t k = 0; k < n; ++k) {
      if (rep_off[k + 1] < rep_off[k]) throw std::runtime_error("report offsets not monotone");
      rep_cnt[k] = rep_off[k + 1] - rep_off[k];
    }
    reply_format_host(n, n ? seg_off : zero, (const SegmentRec*)segs, n ? rep_off : zero, rep_cnt.data(), (const ReportRec*)reps,
                      (const ReportStats*)stats, buf, off, nullptr);
  });
}
int rm_runner_kernel_times(rm_runner* r, double* ms, uint64_t* launches, int n) {
  return guarded([&] {
    double t[kNumKernels];
    uint64_t l[kNumKernels];
    r->m->sync();
    r->m->kernel_times(t, l);
    for (int i = 0; i < n && i < kNumKernels; ++i) { ms[i] = t[i]; if (launches) launches[i] = l[i]; }
  });
}
int rm_runner_reset_times(rm_runner* r) { return guarded([&] { r->m->reset_kernel_times(); }); }
const char* rm_kernel_name(int k) { return (k >= 0 && k < kNumKernels) ? kKernelNames[k] : ""; }
int rm_num_kernels(void) { return kNumKernels; }

}  // extern "C"

struct rm_comm {
  ncclComm_t comm = nullptr;
  hipStream_t stream = nullptr;
  DevBuf<char> scratch;     // 8 bytes for host-value reductions and barriers (freed with the communicator)
  int device = 0;           // -1: a host communicator without a GPU (host values and barriers only)
  int rank = 0, nranks = 1;
  rm_host_allgather_fn host_fn = nullptr;   // set: every collective runs over this host transport
  void* host_ctx = nullptr;
  std::atomic<bool> broken{false};          // a collective missed its deadline (library mode): unusable
};

namespace {
double comm_timeout_s();
// RM_COMM_TIMEOUT_EXIT (default 1): a rank whose peers miss the deadline ends its process with
// status 3 (a failed rank, never a re-exec: what a launcher like torchrun expects); 0 (library
// hosts such as the Python service): the call returns an error instead and the communicator is
// left unusable -- every later call on it fails at once.
bool comm_timeout_exit() {
  const char* e = std::getenv("RM_COMM_TIMEOUT_EXIT");
  return !(e && *e == '0');
}

// The exit-mode watchdog: per calling thread a slot holding the armed call's deadline (0: none),
// polled every 50 ms by one detached thread, started on first use
constexpr uint32_t kWatchSlots = 64;
struct CommWatch {
  std::atomic<uint64_t> deadline_ns[kWatchSlots];
  const char* what[kWatchSlots];
  int rank[kWatchSlots], nranks[kWatchSlots], limit_s[kWatchSlots];
  CommWatch() {
    for (uint32_t i = 0; i < kWatchSlots; ++i) deadline_ns[i].store(0);
  }
};
CommWatch& comm_watch() {
  static CommWatch* w = [] {
    CommWatch* x = new CommWatch();   // (never destroyed: the poller outlives static destruction)
    std::thread([x] {
      for (;;) {
        std::this_thread::sleep_for(std::chrono::milliseconds(50));
        const uint64_t now = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
                                 std::chrono::steady_clock::now().time_since_epoch()).count();
        for (uint32_t i = 0; i < kWatchSlots; ++i) {
          const uint64_t d = x->deadline_ns[i].load(std::memory_order_acquire);
          if (d && now > d) {
            std::fprintf(stderr, "%s: rank %d of %d: the other ranks did not join within %d s (RM_COMM_TIMEOUT_S); "
                                 "exiting with status 3\n", x->what[i], x->rank[i], x->nranks[i], x->limit_s[i]);
            std::fflush(stderr);
            std::_Exit(3);
          }
        }
      }
    }).detach();
    return x;
  }();
  return *w;
}
uint32_t comm_watch_slot() {
  static std::atomic<uint32_t> next{0};
  thread_local const uint32_t slot = next.fetch_add(1) % kWatchSlots;
  return slot;
}

// Every call that waits on the other ranks -- init, the collectives' enqueue and their stream
// wait, a host transport's all-gather -- runs under one deadline, RM_COMM_TIMEOUT_S (VERDICT r05
// item 9: round 5 bounded the init only).  Exit mode: fn runs on this thread and the process-wide
// watchdog (comm_watch) ends the process at the deadline.  Library mode: fn runs on a helper thread that owns everything
// it touches (captured by value); at the deadline this call throws, the communicator is marked
// broken and the helper is left behind, blocked where the peers left it.
template <class F>
void comm_bounded(rm_comm* c, int rank, int nranks, const char* what, F fn) {
  if (c && c->broken.load()) throw std::runtime_error(std::string(what) + ": the communicator missed a deadline earlier and is unusable");
  const double limit = comm_timeout_s();
  struct St {
    std::mutex mu;
    std::condition_variable cv;
    bool done = false;
    std::exception_ptr err;
  };
  auto st = std::make_shared<St>();
  if (comm_timeout_exit()) {
    // one process-wide watchdog thread polls the armed calls' deadlines (a thread per call cost
    // ~40 us per collective: C2's two per-step all-reduces 3.7 -> 89 us)
    CommWatch& w = comm_watch();
    const uint32_t slot = comm_watch_slot();
    w.what[slot] = what;
    w.rank[slot] = rank;
    w.nranks[slot] = nranks;
    w.limit_s[slot] = (int)limit;
    const auto now = std::chrono::steady_clock::now().time_since_epoch();
    w.deadline_ns[slot].store((uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(now).count() +
                              (uint64_t)(limit * 1e9), std::memory_order_release);
    try {
      fn();
    } catch (...) {
      w.deadline_ns[slot].store(0, std::memory_order_release);
      throw;
    }
    w.deadline_ns[slot].store(0, std::memory_order_release);
    return;
  }
  std::thread worker([st, fn]() mutable {
    std::exception_ptr e;
    try {
      fn();
    } catch (...) {
      e = std::current_exception();
    }
    std::lock_guard<std::mutex> lk(st->mu);
    st->err = e;
    st->done = true;
    st->cv.notify_all();
  });
  std::unique_lock<std::mutex> lk(st->mu);
  if (!st->cv.wait_for(lk, std::chrono::duration<double>(limit), [&] { return st->done; })) {
    lk.unlock();
    worker.detach();
    if (c) c->broken = true;
    throw std::runtime_error(std::string(what) + ": no completion within " + std::to_string((int)limit) +
                             " s (RM_COMM_TIMEOUT_S): a rank stopped; the communicator is unusable");
  }
  lk.unlock();
  worker.join();
  if (st->err) std::rethrow_exception(st->err);
}

// every rank's `bytes` host bytes, in rank order (host transport), under the deadline
std::vector<uint8_t> host_gather(rm_comm* c, const void* send, size_t bytes) {
  auto all = std::make_shared<std::vector<uint8_t>>(bytes * (size_t)c->nranks + 1);
  auto mine = std::make_shared<std::vector<uint8_t>>((const uint8_t*)send, (const uint8_t*)send + bytes);
  const rm_host_allgather_fn fn = c->host_fn;
  void* ctx = c->host_ctx;
  comm_bounded(c, c->rank, c->nranks, "host all-gather", [fn, ctx, all, mine, bytes] {
    if (fn(ctx, mine->data(), bytes, all->data()) != 0) throw std::runtime_error("host all-gather failed");
  });
  all->resize(bytes * (size_t)c->nranks);
  return std::move(*all);
}

// element-wise reduction of every rank's buffer in rank order (host transport)
template <class T>
void reduce_ranks(T* dst, const uint8_t* all, size_t count, int nranks, int op) {
  const T* a = (const T*)all;
  for (size_t i = 0; i < count; ++i) {
    T v = a[i];
    for (int r = 1; r < nranks; ++r) {
      const T x = a[(size_t)r * count + i];
      v = op == 0 ? (T)(v + x) : (x > v ? x : v);
    }
    dst[i] = v;
  }
}

void nccl_check(ncclResult_t r, const char* what) {
  if (r != ncclSuccess) throw std::runtime_error(std::string(what) + ": " + ncclGetErrorString(r));
}

// A call that returns ncclInProgress (a non-blocking communicator's; rm_comm_init makes blocking
// ones, so this is a guard) is polled to completion for up to RM_COMM_TIMEOUT_S seconds (default
// 300); past it the communicator is aborted and the call throws.
double comm_timeout_s() {
  const char* e = std::getenv("RM_COMM_TIMEOUT_S");
  const double s = e && *e ? std::atof(e) : 300.0;
  return s > 0.0 ? s : 300.0;
}
void nccl_done(ncclComm_t comm, ncclResult_t r, const char* what) {
  const auto t0 = std::chrono::steady_clock::now();
  const double limit = comm_timeout_s();
  while (r == ncclInProgress) {
    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit) {
      (void)ncclCommAbort(comm);
      throw std::runtime_error(std::string(what) + ": no completion within " + std::to_string((int)limit) +
                               " s (RM_COMM_TIMEOUT_S): a rank did not join; communicator aborted");
    }
    std::this_thread::sleep_for(std::chrono::microseconds(100));
    if (ncclCommGetAsyncError(comm, &r) != ncclSuccess) break;
  }
  nccl_check(r, what);
}

// the tile stage's collectives over RCCL
struct RcclTileComm final : TileComm {
  rm_comm* c;
  ncclComm_t nc;
  void* scratch;
  RcclTileComm(rm_comm* cc) : c(cc), nc(cc->comm), scratch(cc->scratch) { rank = cc->rank; nranks = cc->nranks; }
  uint64_t max_u64(uint64_t v, hipStream_t st) override {
    auto x = std::make_shared<uint64_t>(v);
    ncclComm_t n = nc;
    void* sc = scratch;
    const int dev = c->device;
    comm_bounded(c, rank, nranks, "tile all-reduce", [=] {
      RM_HIP(hipSetDevice(dev));   // (library mode runs this on a helper thread)
      RM_HIP(hipMemcpyAsync(sc, x.get(), 8, hipMemcpyHostToDevice, st));
      nccl_done(n, ncclAllReduce(sc, sc, 1, ncclUint64, ncclMax, n, st), "ncclAllReduce");
      RM_HIP(hipMemcpyAsync(x.get(), sc, 8, hipMemcpyDeviceToHost, st));
      RM_HIP(hipStreamSynchronize(st));
    });
    return *x;
  }
  void allgather(const void* send, void* recv, size_t bytes, hipStream_t st) override {
    ncclComm_t n = nc;
    const int dev = c->device;
    comm_bounded(c, rank, nranks, "tile all-gather", [=] {
      RM_HIP(hipSetDevice(dev));
      nccl_done(n, ncclAllGather(send, recv, bytes, ncclUint8, n, st), "ncclAllGather");
      RM_HIP(hipStreamSynchronize(st));
    });
  }
};

// ... and over an injected host transport (staged through host memory)
struct HostTileComm final : TileComm {
  rm_comm* c;
  explicit HostTileComm(rm_comm* cc) : c(cc) { rank = cc->rank; nranks = cc->nranks; }
  uint64_t max_u64(uint64_t v, hipStream_t) override {
    const std::vector<uint8_t> all = host_gather(c, &v, 8);
    uint64_t m = 0;
    for (int r = 0; r < nranks; ++r) { uint64_t x; std::memcpy(&x, all.data() + 8 * (size_t)r, 8); m = std::max(m, x); }
    return m;
  }
  void allgather(const void* send, void* recv, size_t bytes, hipStream_t st) override {
    std::vector<uint8_t> mine(bytes);
    RM_HIP(hipMemcpyAsync(mine.data(), send, bytes, hipMemcpyDeviceToHost, st));
    RM_HIP(hipStreamSynchronize(st));
    const std::vector<uint8_t> all = host_gather(c, mine.data(), bytes);
    RM_HIP(hipMemcpyAsync(recv, all.data(), all.size(), hipMemcpyHostToDevice, st));
    RM_HIP(hipStreamSynchronize(st));
  }
};

// the tile collectives over a communicator that has a GPU
std::unique_ptr<TileComm> make_tile_comm(rm_comm* comm) {
  if (comm->device < 0) throw std::runtime_error("the communicator has no GPU");
  if (comm->host_fn) return std::make_unique<HostTileComm>(comm);
  return std::make_unique<RcclTileComm>(comm);
}
}  // namespace

extern "C" {

// ---------------- batch-pipeline stages ----------------
int rm_runner_run_points(rm_runner* r, const rm_points_desc* d, const rm_run_params* p) {
  return guarded([&] {
    if (!r || !d) throw std::runtime_error("runner or points descriptor is NULL");
    PointsDesc pd;
    pd.n_points = d->n_points; pd.uuid = d->uuid; pd.time = d->time; pd.lon = d->lon; pd.lat = d->lat;
    pd.accuracy = d->accuracy; pd.inactivity = d->inactivity_sec; pd.n_uuids = d->n_uuids; pd.n_opts = d->n_opts;
    pd.opts = (const MatchOptions*)d->opts; pd.uuid_opt = d->uuid_opt;
    if (pd.n_points && (!pd.uuid || !pd.time || !pd.lon || !pd.lat)) throw std::runtime_error("point arrays are NULL");
    r->m->run_points(pd, to_rp(p));
  });
}
int rm_runner_get_trace_uuid(rm_runner* r, uint32_t* uuid) { return guarded([&] { r->m->get_trace_uuid(uuid); }); }
int rm_runner_get_batch(rm_runner* r, uint32_t* off, float* lon, float* lat, double* time, float* acc) {
  return guarded([&] { r->m->get_batch(off, lon, lat, time, acc); });
}

// ---------------- trace-file text (lines.hip) ----------------
static_assert(sizeof(rm_line_format) == sizeof(sv::Format), "rm_line_format is sv::Format");
void rm_default_line_format(rm_line_format* f) {
  const sv::Format d = sv::default_format();
  std::memcpy(f, &d, sizeof d);
}
int32_t rm_time_pattern(const char* pattern, char* err, size_t errlen) {
  std::string why;
  int32_t id = -1;
  try {
    id = time_pattern_register(pattern, why);
  } catch (const std::exception& e) {
    why = e.what();
  }
  if (id < 0 && err && errlen) std::snprintf(err, errlen, "%s", why.c_str());
  return id;
}
int rm_time_pattern_text(int32_t id, char* out, size_t outlen) {
  const tp::Pattern* p = time_pattern_find(id);
  if (!p) return 1;
  if (out && outlen) std::snprintf(out, outlen, "%s", p->text);
  return 0;
}
int rm_time_pattern_parse(int32_t id, const char* text, size_t n, double* seconds) {
  const tp::Pattern* p = time_pattern_find(id);
  if (!p) return 2;
  double v = 0.0;
  if (!text || n > 0xffff || !tp::match(p->prog, (const uint8_t*)text, (uint32_t)n, v)) return 1;
  if (seconds) *seconds = v;
  return 0;
}
static LinesDesc to_lines(const rm_lines_desc* d) {
  if (!d) throw std::runtime_error("lines descriptor is NULL");
  LinesDesc ld;
  ld.n_chunks = d->n_chunks; ld.data = d->data; ld.len = d->len;
  std::memcpy(&ld.fmt, &d->fmt, sizeof ld.fmt);
  ld.inactivity = d->inactivity_sec; ld.n_opts = d->n_opts; ld.opts = (const MatchOptions*)d->opts;
  return ld;
}
int rm_runner_run_lines(rm_runner* r, const rm_lines_desc* d, const rm_run_params* p) {
  return guarded([&] {
    if (!r) throw std::runtime_error("runner is NULL");
    r->m->run_lines(to_lines(d), to_rp(p));
  });
}
int rm_runner_parse_lines(rm_runner* r, const rm_lines_desc* d) {
  return guarded([&] {
    if (!r) throw std::runtime_error("runner is NULL");
    r->m->parse_lines(to_lines(d));
  });
}
int rm_runner_lines_info(rm_runner* r, uint64_t out[7]) { return guarded([&] { r->m->lines_info(out); }); }
int rm_runner_get_line_points(rm_runner* r, uint32_t* uuid, double* time, float* lon, float* lat, float* acc) {
  return guarded([&] { r->m->get_line_points(uuid, time, lon, lat, acc); });
}
int rm_runner_get_vehicles(rm_runner* r, uint32_t* chunk, uint64_t* off, uint32_t* len) {
  return guarded([&] { r->m->get_vehicles(chunk, off, len); });
}
int rm_runner_lines_time(rm_runner* r, double ms[4]) { return guarded([&] { r->m->lines_time(ms); }); }
int rm_lines_parse_host(const rm_lines_desc* d, uint64_t info[7], uint32_t* uuid, double* time, float* lon, float* lat,
                        float* acc, uint32_t* chunk, uint64_t* off, uint32_t* len, char* err, size_t errlen) {
  const int rc = guarded([&] {
    if (!info) throw std::runtime_error("info is NULL");
    lines_parse_host(to_lines(d), info, uuid, time, lon, lat, acc, chunk, off, len);
  });
  if (rc && err && errlen) {
    std::strncpy(err, g_err.c_str(), errlen - 1);
    err[errlen - 1] = 0;
  }
  return rc;
}

int rm_runner_set_input_coding(rm_runner* r, int coding, int skip_bad) {
  return guarded([&] {
    if (!r) throw std::runtime_error("runner is NULL");
    r->m->set_input_coding(coding, skip_bad != 0);
  });
}
static Matcher& runner_matcher(rm_runner* r) {
  if (!r) throw std::runtime_error("runner is NULL");
  return *r->m;
}
int rm_runner_chunk_count(rm_runner* r, uint32_t* n) {
  return guarded([&] {
    if (!n) throw std::runtime_error("n is NULL");
    *n = runner_matcher(r).chunk_count();
  });
}
int rm_runner_chunk_status(rm_runner* r, uint32_t* status) {
  return guarded([&] {
    Matcher& m = runner_matcher(r);
    if (!status && m.chunk_count()) throw std::runtime_error("status is NULL");
    m.chunk_status(status);
  });
}
int rm_runner_inflate_info(rm_runner* r, uint64_t out[6]) {
  return guarded([&] {
    if (!out) throw std::runtime_error("out is NULL");
    runner_matcher(r).inflate_info(out);
  });
}
int rm_runner_inflate_time(rm_runner* r, double ms[3]) {
  return guarded([&] {
    if (!ms) throw std::runtime_error("ms is NULL");
    runner_matcher(r).inflate_time(ms);
  });
}
int rm_runner_get_text(rm_runner* r, uint32_t chunk, uint64_t off, uint64_t len, char* out) {
  return guarded([&] { runner_matcher(r).get_text(chunk, off, len, out); });
}
// the calling thread's last rm_inflate / rm_inflate_host: members, bytes in, bytes out, second-pass chunks; the times
thread_local uint64_t g_inflate_info[4] = {0, 0, 0, 0};
thread_local double g_inflate_ms[3] = {0.0, 0.0, 0.0};
static int inflate_out(const InflateResult& z, uint32_t n, uint32_t* status, uint64_t* out_len, char** blob, size_t* blob_len,
                       const uint64_t* len) {
  char* b = (char*)std::malloc(std::max<size_t>(z.blob.size(), 1));
  if (!b) return fail("out of memory");
  if (!z.blob.empty()) std::memcpy(b, z.blob.data(), z.blob.size());
  uint64_t members = 0, in = 0;
  for (uint32_t c = 0; c < n; ++c) {
    status[c] = z.status[c];
    out_len[c] = z.off[c + 1] - z.off[c];
    members += z.members[c];
    in += len[c];
  }
  g_inflate_info[0] = members; g_inflate_info[1] = in; g_inflate_info[2] = z.blob.size(); g_inflate_info[3] = z.second_pass;
  std::copy(z.ms, z.ms + 3, g_inflate_ms);
  *blob = b;
  *blob_len = z.blob.size();
  return 0;
}
int rm_inflate(int device, uint32_t n, const char* const* data, const uint64_t* len, uint32_t* status,
               uint64_t* out_len, char** blob, size_t* blob_len) {
  if (!blob || !blob_len || (n && (!status || !out_len))) return fail("inflate: an output argument is NULL");
  *blob = nullptr;
  InflateResult z;
  if (const int rc = guarded([&] { inflate_device(device, n, data, len, z); })) return rc;
  return inflate_out(z, n, status, out_len, blob, blob_len, len);
}
int rm_inflate_host(uint32_t n, const char* const* data, const uint64_t* len, uint32_t* status,
                    uint64_t* out_len, char** blob, size_t* blob_len) {
  if (!blob || !blob_len || (n && (!status || !out_len))) return fail("inflate: an output argument is NULL");
  *blob = nullptr;
  InflateResult z;
  if (const int rc = guarded([&] { inflate_host(n, data, len, z); })) return rc;
  return inflate_out(z, n, status, out_len, blob, blob_len, len);
}
void rm_inflate_last(uint64_t info[4], double ms[3]) {
  if (info) std::copy(g_inflate_info, g_inflate_info + 4, info);
  if (ms) std::copy(g_inflate_ms, g_inflate_ms + 3, ms);
}
const char* rm_inflate_status_text(uint32_t status) { return inf::status_text(status); }

void rm_default_tile_params(rm_tile_params* p) {
  p->quantisation = 3600; p->privacy = 2; p->source = "smpl_rprt"; p->mode = "auto";
}

int rm_runner_tiles(rm_runner* r, const rm_tile_params* p, rm_comm* comm, char** blob, size_t* len) {
  if (!blob || !len) return fail("blob/len is NULL");
  *blob = nullptr;
  *len = 0;
  return guarded([&] {
    if (!r || !p) throw std::runtime_error("runner or tile params is NULL");
    TileParams tp;
    tp.quantisation = p->quantisation;
    tp.privacy = p->privacy;
    tp.source = p->source ? p->source : "";
    std::string mode = p->mode ? p->mode : "auto";
    for (char& ch : mode) ch = (char)std::toupper((unsigned char)ch);   // mode.upper() (:194)
    tp.mode = mode;
    std::unique_ptr<TileComm> tc;
    if (comm) tc = make_tile_comm(comm);
    const std::string out = r->m->tiles(tp, tc.get());
    char* b = (char*)std::malloc(out.size() + 1);
    if (!b) throw std::bad_alloc();
    std::memcpy(b, out.data(), out.size());
    b[out.size()] = 0;
    *blob = b;
    *len = out.size();
  });
}

}  // extern "C"

// ---------------- vehicle sessions (sessions.hip) ----------------
struct rm_session {   // (destroyed in reverse order: the session, then its matcher, then the engine)
  std::shared_ptr<Engine> e;
  std::shared_ptr<Matcher> m;
  std::unique_ptr<Session> s;
  double dir_ms = 0.0;   // the directory's device time in the last rm_session_push_messages
};
static_assert(sizeof(rm_session_report) == sizeof(SessionReport), "rm_session_report is rm::SessionReport");
static_assert(sizeof(rm_session_report) == 56, "rm_session_report layout");
static_assert(sizeof(rm_session_window) == sizeof(SessionWindow), "rm_session_window is rm::SessionWindow");
static_assert(sizeof(rm_session_params) == 112 && sizeof(rm_session_points) == 56, "session descriptors' layout");

extern "C" {

void rm_default_session_params(rm_session_params* p) {
  const SessionParams d;
  p->report_dist_m = d.report_dist_m; p->report_count = d.report_count; p->max_vehicle_points = d.max_vehicle_points;
  p->report_time_s = d.report_time_s; p->session_gap_ms = d.session_gap_ms;
  rm_default_options(&p->opt);
  rm_default_run_params(&p->run);
}

rm_session* rm_session_create(rm_runner* r, uint32_t n_vehicles, const rm_session_params* p) {
  rm_session* out = nullptr;
  guarded([&] {
    if (!r) throw std::runtime_error("runner is NULL");
    SessionParams sp;
    if (p) {
      sp.report_dist_m = p->report_dist_m; sp.report_count = p->report_count; sp.max_vehicle_points = p->max_vehicle_points;
      sp.report_time_s = p->report_time_s; sp.session_gap_ms = p->session_gap_ms;
      std::memcpy(&sp.opt, &p->opt, sizeof sp.opt);
      sp.run = to_rp(&p->run);
    }
    auto s = std::make_unique<rm_session>();
    s->e = r->e;
    s->m = r->m;
    s->s = std::make_unique<Session>(r->m.get(), n_vehicles, sp);
    out = s.release();
  });
  return out;
}
void rm_session_destroy(rm_session* s) { delete s; }

int rm_session_push(rm_session* s, const rm_session_points* pts, uint64_t out[8]) {
  return guarded([&] {
    if (!s || !pts) throw std::runtime_error("session or points is NULL");
    SessionPoints sp;
    sp.n = pts->n; sp.vehicle = pts->vehicle; sp.time = pts->time; sp.lon = pts->lon; sp.lat = pts->lat;
    sp.accuracy = pts->accuracy; sp.stamp_ms = pts->stamp_ms;
    s->s->push(sp, out);
  });
}
int rm_session_punctuate(rm_session* s, int64_t timestamp_ms, uint64_t out[8]) {
  return guarded([&] {
    if (!s) throw std::runtime_error("session is NULL");
    s->s->punctuate(timestamp_ms, out);
  });
}
int rm_session_get_reports(rm_session* s, rm_session_report* out, uint64_t* n) {
  return guarded([&] {
    if (!s) throw std::runtime_error("session is NULL");
    if (n) *n = s->s->n_reports();
    if (out) s->s->get_reports(reinterpret_cast<SessionReport*>(out));
  });
}
int rm_session_get_windows(rm_session* s, rm_session_window* out, uint64_t* n) {
  return guarded([&] {
    if (!s) throw std::runtime_error("session is NULL");
    if (n) *n = s->s->n_windows();
    if (out) s->s->get_windows(reinterpret_cast<SessionWindow*>(out));
  });
}
int rm_session_get_store(rm_session* s, uint32_t* cnt, float* max_sep, int64_t* last_update, float* lon, float* lat,
                         double* time, float* accuracy, uint64_t* n_points) {
  return guarded([&] {
    if (!s) throw std::runtime_error("session is NULL");
    const uint64_t n = s->s->get_store(cnt, max_sep, last_update, lon, lat, time, accuracy);
    if (n_points) *n_points = n;
  });
}
int rm_session_time(rm_session* s, double ms[5]) {
  return guarded([&] {
    if (!s || !ms) throw std::runtime_error("session or ms is NULL");
    s->s->times(ms);
  });
}

}  // extern "C"

// ---------------- stream messages (lines.hip, directory.hip) ----------------
struct rm_directory {
  std::unique_ptr<Directory> d;
};
static_assert(sizeof(rm_message_format) == sizeof(msg::Format), "rm_message_format is msg::Format");
static_assert(sizeof(rm_message_format) == 240 && sizeof(rm_messages_desc) == 280, "message descriptors' layout");

static MessagesDesc to_messages(const rm_messages_desc* d) {
  if (!d) throw std::runtime_error("messages descriptor is NULL");
  MessagesDesc md;
  md.n_chunks = d->n_chunks; md.data = d->data; md.len = d->len;
  std::memcpy(&md.fmt, &d->fmt, sizeof md.fmt);
  md.strict = d->strict; md.has_stamp = d->has_stamp; md.stamp_ms = d->stamp_ms;
  return md;
}
// the listed drops into the C arrays; the reasons NUL-terminated, end to end
static void put_dropped(const std::vector<DroppedMessage>& dr, uint32_t* n, uint32_t* chunk, uint64_t* line, char* reasons,
                        size_t reasons_len) {
  size_t at = 0;
  uint32_t k = 0;
  for (; k < dr.size() && k < 64u; ++k) {
    const size_t w = std::strlen(dr[k].why) + 1;
    if (reasons && at + w > reasons_len) break;
    if (chunk) chunk[k] = dr[k].chunk;
    if (line) line[k] = dr[k].line;
    if (reasons) std::memcpy(reasons + at, dr[k].why, w);
    at += w;
  }
  if (n) *n = k;
}

extern "C" {

void rm_default_message_format(rm_message_format* f) {
  const msg::Format d = msg::default_format();
  std::memcpy(f, &d, sizeof d);
}

rm_directory* rm_directory_create(int device, uint32_t max_vehicles) {
  rm_directory* out = nullptr;
  guarded([&] {
    auto d = std::make_unique<rm_directory>();
    d->d = std::make_unique<Directory>(device, max_vehicles);
    out = d.release();
  });
  return out;
}
void rm_directory_destroy(rm_directory* d) { delete d; }
int rm_directory_size(rm_directory* d, uint32_t* n) {
  return guarded([&] {
    if (!d || !n) throw std::runtime_error("directory or n is NULL");
    *n = d->d->size();
  });
}
int rm_directory_names(rm_directory* d, uint32_t first, uint32_t n, uint64_t* off, char* bytes, uint64_t* n_bytes) {
  return guarded([&] {
    if (!d) throw std::runtime_error("directory is NULL");
    const uint64_t b = d->d->names(first, n, off, bytes);
    if (n_bytes) *n_bytes = b;
  });
}

// nranks 0: the unsharded push
static int push_messages(rm_session* s, rm_directory* dir, const rm_messages_desc* d, int nranks, int rank, uint64_t out[8],
                         uint64_t info[8], uint64_t shard[2]) {
  return guarded([&] {
    if (!s || !dir) throw std::runtime_error("session or directory is NULL");
    if (nranks && (nranks < 1 || rank < 0 || rank >= nranks)) throw std::runtime_error("session shard needs 0 <= rank < nranks");
    if (dir->d->device() != s->s->device()) throw std::runtime_error("the directory is on another device than the session");
    if (dir->d->max_vehicles() > s->s->n_vehicles())
      throw std::runtime_error("the directory's max_vehicles exceeds the session's n_vehicles");
    const MessagesDesc md = to_messages(d);
    Matcher& m = *s->m;
    m.parse_messages(md);
    s->s->check_room(m.line_groups().n_points);   // before the directory is written: a push that cannot fit keys nothing
    dir->d->assign(m);
    s->dir_ms = dir->d->last_ms();
    const LineGroups g = m.line_groups();
    if (nranks)
      s->s->push_device_sharded(g.n_points, g.p_uuid, g.p_time, g.p_lon, g.p_lat, g.p_acc, nullptr, md.has_stamp != 0, md.stamp_ms,
                                nranks, rank, out, shard);
    else
      s->s->push_device(g.n_points, g.p_uuid, g.p_time, g.p_lon, g.p_lat, g.p_acc, nullptr, md.has_stamp != 0, md.stamp_ms, out);
    if (info) {
      m.lines_info(info);
      info[7] = m.dropped_messages(nullptr);
    }
  });
}

int rm_session_push_messages(rm_session* s, rm_directory* dir, const rm_messages_desc* d, uint64_t out[8], uint64_t info[8]) {
  return push_messages(s, dir, d, 0, 0, out, info, nullptr);
}
int rm_session_push_messages_sharded(rm_session* s, rm_directory* dir, const rm_messages_desc* d, int nranks, int rank,
                                     uint64_t out[8], uint64_t info[8], uint64_t shard[2]) {
  if (nranks < 1) return fail("session shard needs 0 <= rank < nranks");
  return push_messages(s, dir, d, nranks, rank, out, info, shard);
}
int rm_vehicle_owner(uint32_t index, int nranks) { return vehicle_owner(index, nranks); }

int rm_session_dropped_messages(rm_session* s, uint32_t* n, uint32_t chunk[64], uint64_t line[64], char* reasons, size_t reasons_len) {
  return guarded([&] {
    if (!s) throw std::runtime_error("session is NULL");
    std::vector<DroppedMessage> dr;
    s->m->dropped_messages(&dr);
    put_dropped(dr, n, chunk, line, reasons, reasons_len);
  });
}

int rm_messages_parse_host(const rm_messages_desc* d, uint64_t info[8], uint32_t* uuid, double* time, float* lon, float* lat,
                           float* acc, uint32_t* chunk, uint64_t* off, uint32_t* len, uint32_t* n_drop, uint32_t drop_chunk[64],
                           uint64_t drop_line[64], char* reasons, size_t reasons_len, char* err, size_t errlen) {
  const int rc = guarded([&] {
    if (!info) throw std::runtime_error("info is NULL");
    std::vector<DroppedMessage> dr;
    messages_parse_host(to_messages(d), info, uuid, time, lon, lat, acc, chunk, off, len, &dr);
    put_dropped(dr, n_drop, drop_chunk, drop_line, reasons, reasons_len);
  });
  if (rc && err && errlen) {
    std::strncpy(err, g_err.c_str(), errlen - 1);
    err[errlen - 1] = 0;
  }
  return rc;
}

int rm_session_messages_span(rm_session* s, double t[2], uint64_t* n_points) {
  return guarded([&] {
    if (!s || !t || !n_points) throw std::runtime_error("session, t or n_points is NULL");
    uint64_t info[7];
    s->m->lines_info(info);
    *n_points = s->m->line_time_span(t) ? info[3] : 0;
  });
}

int rm_session_messages_time(rm_session* s, double ms[9]) {
  return guarded([&] {
    if (!s || !ms) throw std::runtime_error("session or ms is NULL");
    double lt[4] = {0, 0, 0, 0};
    s->m->lines_time(lt);
    ms[0] = lt[0]; ms[1] = lt[1]; ms[2] = lt[2]; ms[3] = s->dir_ms;
    s->s->times(ms + 4);
  });
}

}  // extern "C"

// ---------------- tile store (tilestore.hip) ----------------
struct rm_tilestore {
  std::unique_ptr<TileStore> t;
};
static_assert(sizeof(rm_tile_segment) == sizeof(TileSegment), "rm_tile_segment is rm::TileSegment");

extern "C" {

rm_tilestore* rm_tilestore_create(int device, const rm_tile_params* p, uint64_t initial_rows) {
  rm_tilestore* out = nullptr;
  guarded([&] {
    if (!p) throw std::runtime_error("tile params is NULL");
    TileParams tp;
    tp.quantisation = p->quantisation;
    tp.privacy = p->privacy;
    tp.source = p->source ? p->source : "";
    std::string mode = p->mode ? p->mode : "auto";
    for (char& ch : mode) ch = (char)std::toupper((unsigned char)ch);   // AnonymisingProcessor.java:81
    tp.mode = mode;
    auto t = std::make_unique<rm_tilestore>();
    t->t = std::make_unique<TileStore>(device, tp, initial_rows);
    out = t.release();
  });
  return out;
}
void rm_tilestore_destroy(rm_tilestore* t) { delete t; }

int rm_tilestore_add(rm_tilestore* t, const rm_tile_segment* segs, uint64_t n, uint64_t out[4]) {
  return guarded([&] {
    if (!t) throw std::runtime_error("tile store is NULL");
    t->t->add(reinterpret_cast<const TileSegment*>(segs), n, out);
  });
}
int rm_tilestore_add_session(rm_tilestore* t, rm_session* s, uint64_t out[4]) {
  return guarded([&] {
    if (!t) throw std::runtime_error("tile store is NULL");
    if (!s) throw std::runtime_error("session is NULL");
    t->t->add_session(*s->s, out);
  });
}
int rm_tilestore_flush(rm_tilestore* t, char** blob, size_t* len, uint64_t out[5]) {
  if (!blob || !len) return fail("blob/len is NULL");
  *blob = nullptr;
  *len = 0;
  return guarded([&] {
    if (!t) throw std::runtime_error("tile store is NULL");
    t->t->flush(blob, len, out);
  });
}
int rm_tilestore_time(rm_tilestore* t, double ms[6]) {
  return guarded([&] {
    if (!t || !ms) throw std::runtime_error("tile store or ms is NULL");
    t->t->times(ms);
  });
}

// the sharded stream's exchange (DESIGN.md §3 rule 16)
int rm_tilestore_export_rows(rm_tilestore* t, char** blob, size_t* len) {
  if (!blob || !len) return fail("blob/len is NULL");
  *blob = nullptr;
  *len = 0;
  return guarded([&] {
    if (!t) throw std::runtime_error("tile store is NULL");
    t->t->export_rows(blob, len);
  });
}
int rm_tilestore_import_owned(rm_tilestore* t, const char* const* blobs, const size_t* lens, uint32_t n, int nranks, int rank,
                              uint64_t out[4]) {
  return guarded([&] {
    if (!t) throw std::runtime_error("tile store is NULL");
    t->t->import_owned(blobs, lens, n, nranks, rank, out);
  });
}
int rm_tilestore_exchange(rm_tilestore* t, rm_comm* comm, uint64_t out[4]) {
  return guarded([&] {
    if (!t) throw std::runtime_error("tile store is NULL");
    if (!comm) throw std::runtime_error("communicator is NULL");
    if (comm->device != t->t->device()) throw std::runtime_error("the communicator is on another device than the tile store");
    const std::unique_ptr<TileComm> tc = make_tile_comm(comm);
    t->t->exchange(*tc, out);
  });
}
int rm_tilestore_exchange_time(rm_tilestore* t, double ms[3]) {
  return guarded([&] {
    if (!t || !ms) throw std::runtime_error("tile store or ms is NULL");
    t->t->exchange_times(ms);
  });
}

// ---------------- stream snapshot (snapshot.hpp, snapshot.hip) ----------------
int rm_snapshot_save(rm_session* s, rm_directory* d, rm_tilestore* t, const char* user, size_t user_len, char** blob,
                     size_t* len, uint64_t out[6], double ms[6]) {
  if (!blob || !len) return fail("blob/len is NULL");
  *blob = nullptr;
  *len = 0;
  return guarded([&] { snapshot_save(s ? s->s.get() : nullptr, d ? d->d.get() : nullptr, t ? t->t.get() : nullptr, user, user_len, blob, len, out, ms); });
}
int rm_snapshot_load(rm_session* s, rm_directory* d, rm_tilestore* t, const char* blob, size_t len, uint64_t out[6],
                     double ms[6]) {
  return guarded([&] {
    if (!blob) throw std::runtime_error("blob is NULL");
    snapshot_load(s ? s->s.get() : nullptr, d ? d->d.get() : nullptr, t ? t->t.get() : nullptr, blob, len, out, ms);
  });
}
int rm_snapshot_check_host(const char* blob, size_t len, uint64_t info[9], char* err, size_t errlen) {
  const int rc = guarded([&] {
    const std::string why = snap::check_host(blob, len, info);
    if (!why.empty()) throw std::runtime_error(why);
  });
  if (rc && err && errlen) {
    std::strncpy(err, g_err.c_str(), errlen - 1);
    err[errlen - 1] = 0;
  }
  return rc;
}

// the snapshot of a stream on several ranks (DESIGN.md §3 rule 17)
int rm_snapshot_save_shard(rm_session* s, rm_directory* d, rm_tilestore* t, int rank, int nranks, const char* user,
                           size_t user_len, char** blob, size_t* len, uint64_t out[6], double ms[6]) {
  if (!blob || !len) return fail("blob/len is NULL");
  *blob = nullptr;
  *len = 0;
  return guarded([&] {
    snapshot_save_shard(s ? s->s.get() : nullptr, d ? d->d.get() : nullptr, t ? t->t.get() : nullptr, rank, nranks, user, user_len,
                        blob, len, out, ms);
  });
}
int rm_snapshot_load_shards(rm_session* s, rm_directory* d, rm_tilestore* t, const char* const* blobs, const size_t* lens,
                            uint32_t n_blobs, int rank, int nranks, uint64_t out[8], double ms[6]) {
  return guarded([&] {
    snapshot_load_shards(s ? s->s.get() : nullptr, d ? d->d.get() : nullptr, t ? t->t.get() : nullptr, blobs, lens, n_blobs, rank,
                         nranks, out, ms);
  });
}
int rm_snapshot_check_host_shard(const char* blob, size_t len, uint64_t info[12], char* err, size_t errlen) {
  const int rc = guarded([&] {
    const std::string why = snap::check_host(blob, len, info, 0, info ? info + 9 : nullptr);
    if (!why.empty()) throw std::runtime_error(why);
  });
  if (rc && err && errlen) {
    std::strncpy(err, g_err.c_str(), errlen - 1);
    err[errlen - 1] = 0;
  }
  return rc;
}

}  // extern "C"

namespace {
}  // namespace

extern "C" {

int rm_comm_unique_id(uint8_t id_out[128]) {
  return guarded([&] {
    ncclUniqueId id;
    nccl_check(ncclGetUniqueId(&id), "ncclGetUniqueId");
    std::memcpy(id_out, id.internal, NCCL_UNIQUE_ID_BYTES);
  });
}

rm_comm* rm_comm_init(int nranks, int rank, const uint8_t id[128], int device) {
  rm_comm* out = nullptr;
  guarded([&] {
    auto c = std::make_unique<rm_comm>();
    c->device = device;
    c->rank = rank;
    c->nranks = nranks;
    RM_HIP(hipSetDevice(device));
    ncclUniqueId uid;
    std::memcpy(uid.internal, id, NCCL_UNIQUE_ID_BYTES);
    // A bounded wait for the peers: a rank whose peers never join (a crashed
    // launch, a stale rendezvous id) must fail, not block in the init forever.  RCCL's init cannot
    // be cancelled once its bootstrap waits for the peers (aborting a non-blocking init hung in
    // tests), so at RM_COMM_TIMEOUT_S seconds (default 300) the process ends with status 3, or
    // (RM_COMM_TIMEOUT_EXIT=0) this call fails and the blocked init is left behind (comm_bounded).
    auto res = std::make_shared<std::pair<ncclComm_t, ncclResult_t>>(nullptr, ncclSuccess);
    comm_bounded(nullptr, rank, nranks, "rm_comm_init", [=] {
      RM_HIP(hipSetDevice(device));
      res->second = ncclCommInitRank(&res->first, nranks, uid, rank);
    });
    const ncclResult_t r = res->second;
    c->comm = r == ncclSuccess ? res->first : nullptr;
    nccl_check(r, "ncclCommInitRank");
    RM_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    c->scratch.reserve(8);
    out = c.release();
  });
  return out;
}

rm_comm* rm_comm_init_host(int nranks, int rank, rm_host_allgather_fn fn, void* ctx, int device) {
  rm_comm* out = nullptr;
  guarded([&] {
    if (!fn) throw std::runtime_error("host all-gather function is NULL");
    if (nranks < 1 || rank < 0 || rank >= nranks) throw std::runtime_error("bad rank / nranks");
    auto c = std::make_unique<rm_comm>();
    c->device = device;
    c->rank = rank;
    c->nranks = nranks;
    c->host_fn = fn;
    c->host_ctx = ctx;
    if (device >= 0) {
      RM_HIP(hipSetDevice(device));
      RM_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
      c->scratch.reserve(8);
    }
    out = c.release();
  });
  return out;
}

int rm_tile_file_owner(uint64_t bucket, uint32_t tile, int nranks) { return tile_file_owner(bucket, tile, nranks); }

void rm_comm_destroy(rm_comm* c) {
  if (!c) return;
  if (c->device >= 0) (void)hipSetDevice(c->device);
  if (c->comm) ncclCommDestroy(c->comm);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

// host transport: reduce elements [lo, lo + count) of every rank's n-element buffer (gathered
// whole) into dst; a device -1 communicator's buffers are host memory
static void host_reduce_range(rm_comm* c, void* buf, size_t n, size_t lo, size_t count, int dtype, int op) {
  const size_t es = dtype == 0 ? 4 : 8, bytes = es * n;
  std::vector<uint8_t> mine(bytes);
  if (c->device >= 0) {
    RM_HIP(hipSetDevice(c->device));
    RM_HIP(hipMemcpy(mine.data(), buf, bytes, hipMemcpyDeviceToHost));
  } else if (bytes) {
    std::memcpy(mine.data(), buf, bytes);
  }
  const std::vector<uint8_t> all = host_gather(c, mine.data(), bytes);
  // rank r's element i sits at all[r * bytes + i * es]; reduce_ranks reads all + r * (count * es)
  std::vector<uint8_t> part((size_t)c->nranks * count * es);
  for (int r = 0; r < c->nranks; ++r)
    if (count) std::memcpy(part.data() + (size_t)r * count * es, all.data() + (size_t)r * bytes + lo * es, count * es);
  uint8_t* dst = mine.data() + lo * es;
  if (dtype == 0) reduce_ranks((uint32_t*)dst, part.data(), count, c->nranks, op);
  else if (dtype == 1) reduce_ranks((uint64_t*)dst, part.data(), count, c->nranks, op);
  else reduce_ranks((double*)dst, part.data(), count, c->nranks, op);
  if (!count) return;
  if (c->device >= 0) RM_HIP(hipMemcpy((uint8_t*)buf + lo * es, dst, count * es, hipMemcpyHostToDevice));
  else std::memcpy((uint8_t*)buf + lo * es, dst, count * es);
}

int rm_comm_allreduce(rm_comm* c, void* buf, size_t count, int dtype, int op) {
  return guarded([&] {
    if (!c) throw std::runtime_error("comm is NULL");
    if (dtype < 0 || dtype > 2 || op < 0 || op > 1) throw std::runtime_error("bad dtype / op");
    if (c->host_fn) {
      host_reduce_range(c, buf, count, 0, count, dtype, op);
      return;
    }
    const ncclDataType_t dt = dtype == 0 ? ncclUint32 : (dtype == 1 ? ncclUint64 : ncclFloat64);
    const ncclRedOp_t ro = op == 0 ? ncclSum : ncclMax;
    const int dev = c->device;
    ncclComm_t nc = c->comm;
    hipStream_t cs = c->stream;
    comm_bounded(c, c->rank, c->nranks, "rm_comm_allreduce", [=] {
      RM_HIP(hipSetDevice(dev));
      nccl_done(nc, ncclAllReduce(buf, buf, count, dt, ro, nc, cs), "ncclAllReduce");
      RM_HIP(hipStreamSynchronize(cs));
    });
  });
}

int rm_comm_reduce_scatter(rm_comm* c, void* buf, size_t count_per_rank, int dtype, int op) {
  return guarded([&] {
    if (!c) throw std::runtime_error("comm is NULL");
    if (dtype < 0 || dtype > 2 || op < 0 || op > 1) throw std::runtime_error("bad dtype / op");
    const size_t lo = (size_t)c->rank * count_per_rank, n = (size_t)c->nranks * count_per_rank;
    if (c->host_fn) {
      host_reduce_range(c, buf, n, lo, count_per_rank, dtype, op);
      return;
    }
    const ncclDataType_t dt = dtype == 0 ? ncclUint32 : (dtype == 1 ? ncclUint64 : ncclFloat64);
    const size_t es = dtype == 0 ? 4 : 8;
    const int dev = c->device;
    ncclComm_t nc = c->comm;
    hipStream_t cs = c->stream;
    comm_bounded(c, c->rank, c->nranks, "rm_comm_reduce_scatter", [=] {
      RM_HIP(hipSetDevice(dev));
      // in place: this rank's chunk of the nranks-chunk buffer receives the reduction
      nccl_done(nc, ncclReduceScatter(buf, (uint8_t*)buf + lo * es, count_per_rank, dt, op == 0 ? ncclSum : ncclMax, nc, cs),
                "ncclReduceScatter");
      RM_HIP(hipStreamSynchronize(cs));
    });
  });
}

int rm_comm_allreduce_host_f64(rm_comm* c, double* value, int op) {
  return guarded([&] {
    if (!c) throw std::runtime_error("comm is NULL");
    if (c->host_fn) {
      const std::vector<uint8_t> all = host_gather(c, value, 8);
      reduce_ranks(value, all.data(), 1, c->nranks, op);
      return;
    }
    const int dev = c->device;
    ncclComm_t nc = c->comm;
    hipStream_t cs = c->stream;
    void* scratch = c->scratch;
    auto v = std::make_shared<double>(*value);
    comm_bounded(c, c->rank, c->nranks, "rm_comm_allreduce_host_f64", [=] {
      RM_HIP(hipSetDevice(dev));
      RM_HIP(hipMemcpyAsync(scratch, v.get(), 8, hipMemcpyHostToDevice, cs));
      nccl_done(nc, ncclAllReduce(scratch, scratch, 1, ncclFloat64, op == 0 ? ncclSum : ncclMax, nc, cs), "ncclAllReduce");
      RM_HIP(hipMemcpyAsync(v.get(), scratch, 8, hipMemcpyDeviceToHost, cs));
      RM_HIP(hipStreamSynchronize(cs));
    });
    *value = *v;
  });
}

int rm_comm_barrier(rm_comm* c) {
  double one = 1.0;
  const int rc = rm_comm_allreduce_host_f64(c, &one, 0);
  if (rc == 0 && c->device >= 0) {
    return guarded([&] { RM_HIP(hipDeviceSynchronize()); });
  }
  return rc;
}

int rm_device_alloc(size_t bytes, void** p) { return guarded([&] { RM_HIP(hipMalloc(p, bytes)); }); }
int rm_device_free(void* p) { return guarded([&] { RM_HIP(hipFree(p)); }); }
int rm_device_memset(void* p, int v, size_t n) { return guarded([&] { RM_HIP(hipMemset(p, v, n)); }); }
int rm_device_download(void* dst, const void* src, size_t n) {
  return guarded([&] { RM_HIP(hipMemcpy(dst, src, n, hipMemcpyDeviceToHost)); });
}
int rm_device_upload(void* dst, const void* src, size_t n) {
  return guarded([&] { RM_HIP(hipMemcpy(dst, src, n, hipMemcpyHostToDevice)); });
}
int rm_device_synchronize(void) { return guarded([&] { RM_HIP(hipDeviceSynchronize()); }); }

}  // extern "C"
