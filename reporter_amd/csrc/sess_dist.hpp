// sess_dist.hpp — the distance and trigger rule of the vehicle sessions (DESIGN.md §3 rule 12),
// shared by k_sess_trigger (sessions.hip) and the host test (tests/cpp/sess_dist_test.cpp).
#pragma once
#include <cstdint>

#include "rm_common.hpp"

namespace rm {

constexpr double kSessMetersPerDeg = 20037581.187 / 180.0;   // Batch.java:36

// Batch.java:37-41 in Java's types: the longitude difference and the latitude mean are float
// operations, everything after them is double; cos is det_cos (the stated deviation from Math.cos)
RM_HD double sess_distance(float alon, float alat, float blon, float blat) {
  const float dlon = alon - blon, dlat = alat - blat;
  const float mean = 0.5f * (alat + blat);
  const double x = (double)dlon * kSessMetersPerDeg * det_cos((double)mean * kDegToRad);
  const double y = (double)dlat * kSessMetersPerDeg;
  return __builtin_sqrt(x * x + y * y);
}

// max_sep = (float)max((double)max_sep, d) (Batch.java:45) == max(max_sep, (float)d): rounding to
// float is monotone, so the running maximum is a prefix maximum of the rounded distances
RM_HD float sess_fold(float max_sep, double d) {
  const float f = (float)d;
  return f > max_sep ? f : max_sep;
}

// the bail of Batch.java:51-53, negated: a list of n points whose first and last times are t0, tl
RM_HD bool sess_reports(float max_sep, uint32_t n, double t0, double tl, double dist_m, uint32_t count, double time_s) {
  return !((double)max_sep < dist_m || n < count || tl - t0 < time_s);
}

}  // namespace rm
