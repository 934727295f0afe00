// match_options.report_levels / transition_levels as the request reader takes them for the Report
// calls (reporter_amd/csrc/trace_json.hpp parse_report_request; DESIGN.md §3 rule 19): the masks,
// the first match_options winning, the failures and their texts, and the Match reading of the same
// requests, which ignores both keys.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "trace_json.hpp"

using namespace rm;

static int g_fail = 0;
#define CHECK(c)                                                          \
  do {                                                                    \
    if (!(c)) {                                                           \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);             \
      if (++g_fail > 20) std::exit(1);                                    \
    }                                                                     \
  } while (0)

static const char* kTrace = "\"trace\":[{\"lat\":47.1,\"lon\":8.1,\"time\":100},{\"lat\":47.2,\"lon\":8.2,\"time\":101.5}]";

struct Out {
  std::string err;
  tj::ReportLevels lv;
  size_t points = 0;
  MatchOptions opt;
};

static Out as_report(const std::string& text, bool deferred = false) {
  MatchOptions defaults[5];
  for (int m = 0; m < 5; ++m) { defaults[m] = default_options(); defaults[m].mode = m; }
  Out o;
  tj::PointSink sink;
  tj::TraceSpan sp;
  try {
    o.opt = tj::parse_report_request(text.c_str(), text.size(), defaults, sink, o.lv, deferred ? &sp : nullptr);
  } catch (const std::exception& e) {
    o.err = e.what();
  }
  o.points = sink.size() + (sp.on ? sp.n_open : 0);
  return o;
}
static Out as_match(const std::string& text) {
  MatchOptions defaults[5];
  for (int m = 0; m < 5; ++m) { defaults[m] = default_options(); defaults[m].mode = m; }
  Out o;
  tj::PointSink sink;
  try {
    o.opt = tj::parse_request(text.c_str(), text.size(), defaults, sink);
  } catch (const std::exception& e) {
    o.err = e.what();
  }
  o.points = sink.size();
  return o;
}
static std::string req(const std::string& options) { return std::string("{\"uuid\":\"u\",") + kTrace + options + "}"; }

int main() {
  // ---- masks: bit (level + 1) per integer entry in -1..7, other numbers nothing
  struct { const char* r; const char* t; uint32_t rm, tm; } good[] = {
      {"[0,1]", "[0,1]", 0b0110, 0b0110},
      {"[0,1,2]", "[0, 1 ,2]", 0b1110, 0b1110},
      {"[]", "[0,1]", 0, 0b0110},
      {"[2]", "[]", 0b1000, 0},
      {"[0,1]", "[-1,0,1,2]", 0b0110, 0b1111},
      {"[7,7,0]", "[8,-2,1.5,1e0,2.0]", 0b100000010, 0b1100},
      {"[1e300,-1e300,0.0]", "[-0.0,3]", 0b10, 0b10010},
  };
  for (const auto& g : good) {
    const std::string text = req(std::string(",\"match_options\":{\"mode\":\"auto\",\"report_levels\":") + g.r +
                                 ",\"transition_levels\":" + g.t + ",\"sigma_z\":5}");
    for (int deferred = 0; deferred < 2; ++deferred) {
      const Out o = as_report(text, deferred != 0);
      CHECK(o.err.empty());
      CHECK(o.lv.report_mask == g.rm && o.lv.transition_mask == g.tm);
      CHECK(o.points == 2 && o.opt.sigma_z == 5.f);
    }
    const Out m = as_match(text);
    CHECK(m.err.empty() && m.points == 2 && m.opt.sigma_z == 5.f);
  }
  // ---- the first match_options and, inside it, the first of either key win
  {
    const Out o = as_report(req(",\"match_options\":{\"report_levels\":[0],\"report_levels\":[1],\"transition_levels\":[2],"
                                "\"transition_levels\":\"x\"},\"match_options\":{\"report_levels\":[5],\"transition_levels\":[5]}"));
    CHECK(o.err.empty() && o.lv.report_mask == 0b10 && o.lv.transition_mask == 0b1000);
    const Out p = as_report(req(",\"match_options\":{},\"match_options\":{\"report_levels\":[0],\"transition_levels\":[0]}"));
    CHECK(p.err == "match_options must include report_levels array");
  }
  // ---- failures: the service's texts for a missing or non-array value, a non-number entry named
  struct { const char* options; const char* err; } bad[] = {
      {"", "match_options must include report_levels array"},
      {",\"match_options\":5", "match_options must include report_levels array"},
      {",\"match_options\":{\"transition_levels\":[0]}", "match_options must include report_levels array"},
      {",\"match_options\":{\"report_levels\":null,\"transition_levels\":[0]}", "match_options must include report_levels array"},
      {",\"match_options\":{\"report_levels\":{\"0\":1},\"transition_levels\":[0]}", "match_options must include report_levels array"},
      {",\"match_options\":{\"report_levels\":\"0,1\",\"transition_levels\":[0]}", "match_options must include report_levels array"},
      {",\"match_options\":{\"report_levels\":[0,1]}", "match_options must include transition_levels array"},
      {",\"match_options\":{\"report_levels\":[0,1],\"transition_levels\":7}", "match_options must include transition_levels array"},
      {",\"match_options\":{\"report_levels\":[0,\"1\"],\"transition_levels\":[0]}", "report_levels entries must be numbers"},
      {",\"match_options\":{\"report_levels\":[null],\"transition_levels\":[0]}", "report_levels entries must be numbers"},
      {",\"match_options\":{\"report_levels\":[0],\"transition_levels\":[[0]]}", "transition_levels entries must be numbers"},
      {",\"match_options\":{\"report_levels\":[true],\"transition_levels\":[\"a\"]}", "report_levels entries must be numbers"},
  };
  for (const auto& b : bad) {
    const std::string text = req(b.options);
    for (int deferred = 0; deferred < 2; ++deferred) {
      const Out o = as_report(text, deferred != 0);
      CHECK(o.err == b.err);
      if (!deferred) CHECK(o.points == 0);   // nothing appended by a failed request
    }
    const Out m = as_match(text);   // Match of the same text: unaffected by those keys
    CHECK(m.err.empty() && m.points == 2);
  }
  // ---- what fails as a Match request fails with that error first, with its text unchanged
  {
    const char* both[] = {
        "{\"uuid\":\"u\",\"trace\":[],\"match_options\":{}}",
        "{\"uuid\":\"u\",\"trace\":[{\"lat\":47.1,\"lon\":8.1,\"time\":1}],\"match_options\":{\"mode\":\"boat\"}}",
        "{\"uuid\":\"u\",\"trace\":[{\"lat\":47.1,\"lon\":8.1,\"time\":1}],\"match_options\":{\"sigma_z\":\"x\",\"report_levels\":3}}",
        "{\"uuid\":\"u\",\"trace\":[{\"lat\":47.1,\"lon\":8.1,\"time\":1}],\"match_options\":{\"report_levels\":[0,]}}",
        "[1,2]",
    };
    for (const char* t : both) {
      const Out o = as_report(t), m = as_match(t);
      CHECK(!m.err.empty() && o.err == m.err);
    }
  }
  if (g_fail) return 1;
  std::printf("report levels ok\n");
  return 0;
}
