// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text; functional).
//
// Restates the slice of PCL 1.10 common/include/pcl/point_cloud.h the reference touches: a vector of points with header / width /
// height / is_dense, Ptr = boost::shared_ptr, push_back (width = size, height = 1), clear (width = height = 0), operator+= (append;
// the result is dense only if both operands are; width = size, height = 1) and size().  A default-constructed cloud is dense
// (is_dense = true), as in PCL.
// One addition of our own, for observation only: refshim_appended logs the size of every cloud that operator+= appended since the last
// clear(), so that a reader of the joined cloud (the published /laser_cloud_map) can tell its parts apart.  No arithmetic depends on it.
#pragma once
#include <boost/make_shared.hpp>
#include <boost/shared_ptr.hpp>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace pcl {

struct PCLHeader {
  std::uint32_t seq = 0;
  std::uint64_t stamp = 0;
  std::string frame_id;
};

template <class PointT>
class PointCloud {
 public:
  typedef boost::shared_ptr<PointCloud<PointT>> Ptr;
  typedef boost::shared_ptr<const PointCloud<PointT>> ConstPtr;

  PCLHeader header;
  std::vector<PointT> points;
  std::uint32_t width = 0, height = 0;
  bool is_dense = true;
  std::vector<std::uint32_t> refshim_appended;

  std::size_t size() const { return points.size(); }
  bool empty() const { return points.empty(); }
  void clear() { points.clear(); width = 0; height = 0; refshim_appended.clear(); }
  void push_back(const PointT& p) { points.push_back(p); width = static_cast<std::uint32_t>(points.size()); height = 1; }
  PointT& operator[](std::size_t i) { return points[i]; }
  const PointT& operator[](std::size_t i) const { return points[i]; }

  PointCloud& operator+=(const PointCloud& rhs) {
    if (rhs.header.stamp > header.stamp) header.stamp = rhs.header.stamp;
    points.insert(points.end(), rhs.points.begin(), rhs.points.end());
    refshim_appended.push_back(static_cast<std::uint32_t>(rhs.points.size()));
    width = static_cast<std::uint32_t>(points.size());
    height = 1;
    is_dense = is_dense && rhs.is_dense;
    return *this;
  }
};

}  // namespace pcl
