// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).
// pcl::toROSMsg copies the points (x, y, z, intensity where the type has one) and the append log into the stand-in message, so that a
// published cloud can be read back; pcl::fromROSMsg is never reached by the files built here and does nothing.
#pragma once
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#include <sensor_msgs/PointCloud2.h>

namespace pcl {
namespace refshim {
inline float intensity_of(const PointXYZI& p) { return p.intensity; }
inline float intensity_of(const PointXYZ&) { return 0.f; }
}  // namespace refshim
template <class PointT> inline void toROSMsg(const PointCloud<PointT>& c, sensor_msgs::PointCloud2& m) {
  m.xyzi.resize(4 * c.points.size());
  for (std::size_t i = 0; i < c.points.size(); i++) {
    m.xyzi[4 * i] = c.points[i].x; m.xyzi[4 * i + 1] = c.points[i].y; m.xyzi[4 * i + 2] = c.points[i].z;
    m.xyzi[4 * i + 3] = refshim::intensity_of(c.points[i]);
  }
  m.appended = c.refshim_appended;
}
template <class PointT> inline void fromROSMsg(const sensor_msgs::PointCloud2&, PointCloud<PointT>&) {}
}  // namespace pcl
