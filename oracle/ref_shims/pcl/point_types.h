// oracle/ref_shims/pcl/point_types.h - a stand-in for pcl::PointXYZ and pcl::PointCloud as the reference's
// mc_ring/operations.h uses them (a vector of points behind a shared pointer).  TEST INFRASTRUCTURE ONLY, for
// oracle/ref_harness.cpp.  No arithmetic happens here.
#pragma once
#include <cstddef>
#include <memory>
#include <vector>

namespace pcl {

struct PointXYZ {
  float x = 0.f, y = 0.f, z = 0.f;
};

template <class P> class PointCloud {
 public:
  typedef std::shared_ptr<PointCloud<P>> Ptr;
  std::vector<P> points;
  size_t size() const { return points.size(); }
  void clear() { points.clear(); }
  void reserve(size_t n) { points.reserve(n); }
  void push_back(const P &p) { points.push_back(p); }
};

}  // namespace pcl
