// interval_union.h -- the measure of a union of intervals that arrive roughly in order, in bounded memory; host-only
// C++ (no HIP).  timeline.cpp keeps one per launch kind; tools/host_asan_main.cpp (tests/test_sanitizers_cpu.py)
// drives it under ASan + UBSan.
#pragma once
#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

namespace uc {

// Once more than `cap` intervals are held they are merged, and all but the latest `keep` merged ones are folded into a
// running sum, so that a long run does not grow the vector without bound.  fold_hi is the end of the last folded
// interval: a later interval is clipped there, so one that arrives late counts only for what lies above fold_hi --
// `keep` is the allowance for late arrivals.
struct IntervalUnion {
  const size_t cap, keep;
  std::vector<std::pair<float, float>> iv;
  double folded = 0.0;     // measure of the folded intervals
  float fold_hi = -1e30f;

  IntervalUnion(size_t cap_, size_t keep_) : cap(cap_), keep(keep_) {}

  void clear() {
    iv.clear();
    folded = 0.0;
    fold_hi = -1e30f;
  }
  void add(float t0, float t1) {
    t0 = std::max(t0, fold_hi);
    if (t1 <= t0) return;
    iv.emplace_back(t0, t1);
    if (iv.size() > cap) {
      merge(iv);
      if (iv.size() > keep) {
        const size_t f = iv.size() - keep;
        for (size_t i = 0; i < f; i++) folded += iv[i].second - iv[i].first;
        fold_hi = iv[f - 1].second;
        iv.erase(iv.begin(), iv.begin() + (ptrdiff_t)f);
      }
    }
  }
  double measure() const {
    std::vector<std::pair<float, float>> v = iv;
    return folded + merge(v);
  }

  // union of intervals: sorts and merges v in place, returns the measure
  static double merge(std::vector<std::pair<float, float>>& v) {
    std::sort(v.begin(), v.end());
    size_t w = 0;
    double tot = 0.0;
    for (size_t i = 0; i < v.size(); i++) {
      if (w > 0 && v[i].first <= v[w - 1].second) {
        v[w - 1].second = std::max(v[w - 1].second, v[i].second);
      } else {
        v[w++] = v[i];
      }
    }
    v.resize(w);
    for (const auto& x : v) tot += x.second - x.first;
    return tot;
  }
};

}  // namespace uc
