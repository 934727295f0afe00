// The host side of the vehicle sessions' distance and trigger rule (sess_dist.hpp; DESIGN.md §3
// rule 12): Java's float maximum is a maximum of floats, a 16-wide prefix maximum seeded with the
// carried value finds the arrival the sequential rule finds, and the distance is the expression of
// Batch.java:37-41 in Java's types.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "sess_dist.hpp"

using namespace rm;

static int fails = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } \
  } while (0)

// the arrival loop as Batch.update / Batch.report write it: first list index in [try_from, n) at
// which the three-part condition holds, or n
static uint32_t sequential(const std::vector<double>& d, const std::vector<double>& t, float seed, uint32_t scan_from,
                           uint32_t try_from, double dist, uint32_t count, double time_s, float& max_sep) {
  max_sep = seed;
  const uint32_t n = (uint32_t)d.size();
  for (uint32_t i = scan_from; i < n; ++i) {
    max_sep = (float)std::fmax((double)max_sep, d[i]);
    if (i >= try_from && !((double)max_sep < dist || i + 1 < count || t[i] - t[0] < time_s)) return i;
  }
  return n;
}

// the same in steps of 16 lanes: an inclusive prefix maximum of the rounded distances per step
static uint32_t stepped(const std::vector<double>& d, const std::vector<double>& t, float seed, uint32_t scan_from,
                        uint32_t try_from, double dist, uint32_t count, double time_s, float& max_sep) {
  float m = seed;
  const uint32_t n = (uint32_t)d.size();
  for (uint32_t base = scan_from; base < n; base += 16) {
    float pm[16];
    for (uint32_t l = 0; l < 16; ++l) pm[l] = base + l < n ? (float)d[base + l] : 0.0f;
    for (uint32_t s = 1; s < 16; s <<= 1)
      for (uint32_t l = 15; l >= s; --l)
        if (pm[l - s] > pm[l]) pm[l] = pm[l - s];
    for (uint32_t l = 0; l < 16; ++l) {
      if (m > pm[l]) pm[l] = m;
      const uint32_t i = base + l;
      if (i < n && i >= try_from && sess_reports(pm[l], i + 1, t[0], t[i], dist, count, time_s)) {
        max_sep = pm[l];
        return i;
      }
    }
    m = pm[15];
  }
  max_sep = m;
  return n;
}

int main() {
  std::mt19937_64 rng(12);
  std::uniform_real_distribution<double> U(0.0, 3000.0), E(-1e-4, 1e-4);
  for (int k = 0; k < 200000; ++k) {
    const float m = (float)U(rng);
    const double d = (k & 1) ? U(rng) : (double)m + E(rng);   // around the rounding boundaries too
    CHECK(sess_fold(m, d) == (float)std::fmax((double)m, d));
  }
  for (int k = 0; k < 4000; ++k) {
    const uint32_t n = 1 + (uint32_t)(rng() % 90);
    std::vector<double> d(n), t(n);
    const double scale = (k % 3) ? 12.0 : 2.0;
    for (uint32_t i = 0; i < n; ++i) { d[i] = scale * i + U(rng) / 100.0; t[i] = 100.0 + i + ((k % 7) ? 0.0 : E(rng) * 1e4); }
    const uint32_t scan_from = 1 + (uint32_t)(rng() % 3), try_from = scan_from + (uint32_t)(rng() % 20);
    const float seed = (k % 5) ? 0.0f : (float)U(rng) / 10.0f;
    const uint32_t count = 2 + (uint32_t)(rng() % 30);
    float a = 0, b = 0;
    const uint32_t ia = sequential(d, t, seed, scan_from, try_from, 500.0, count, 40.0, a);
    const uint32_t ib = stepped(d, t, seed, scan_from, try_from, 500.0, count, 40.0, b);
    CHECK(ia == ib);
    CHECK(a == b);
  }
  // the distance: along a meridian it is the latitude difference in Java's metres per degree
  const float lat0 = 14.5f, lat1 = 14.5001f, lon = 121.0f;
  CHECK(sess_distance(lon, lat1, lon, lat0) == (double)(lat1 - lat0) * kSessMetersPerDeg);
  CHECK(sess_distance(lon, lat0, lon, lat0) == 0.0);
  {
    const float lon1 = 121.01f;
    const double x = (double)(lon1 - lon) * kSessMetersPerDeg * det_cos((double)(0.5f * (lat0 + lat1)) * kDegToRad);
    const double y = (double)(lat1 - lat0) * kSessMetersPerDeg;
    CHECK(sess_distance(lon1, lat1, lon, lat0) == std::sqrt(x * x + y * y));
    CHECK(sess_distance(lon1, lat1, lon, lat0) == sess_distance(lon, lat0, lon1, lat1));
    CHECK(std::fabs(sess_distance(lon1, lat0, lon, lat0) - 1077.7) < 2.0);
  }
  // the bail, at each threshold's edge (Batch.java:51-53)
  CHECK(sess_reports(500.0f, 10, 0.0, 60.0, 500.0, 10, 60.0));
  CHECK(!sess_reports(499.99997f, 10, 0.0, 60.0, 500.0, 10, 60.0));
  CHECK(!sess_reports(500.0f, 9, 0.0, 60.0, 500.0, 10, 60.0));
  CHECK(!sess_reports(500.0f, 10, 0.0, 59.999, 500.0, 10, 60.0));
  CHECK(sess_reports(0.0f, 2, 5.0, 5.0, 0.0, 2, 0.0));
  CHECK(!sess_reports(0.0f, 2, 5.0, 4.0, 0.0, 2, 0.0));   // eviction still bails on negative elapsed time
  if (fails) return 1;
  std::printf("sess dist ok\n");
  return 0;
}
