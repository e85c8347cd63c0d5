// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text; functional).
//
// Restates pcl::removeNaNFromPointCloud of PCL 1.10 (filters/include/pcl/filters/impl/filter.hpp), INCLUDING the early-out the
// oracle's C ABI cannot reach: a cloud whose is_dense flag is set is copied as it is, without looking at a single coordinate; only a
// cloud flagged non-dense has its non-finite points (x, y or z) removed, after which the output is flagged dense.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>
#include <pcl/point_cloud.h>

namespace pcl {

template <class PointT>
void removeNaNFromPointCloud(const PointCloud<PointT>& cloud_in, PointCloud<PointT>& cloud_out, std::vector<int>& index) {
  if (&cloud_in != &cloud_out) {
    cloud_out.header = cloud_in.header;
    cloud_out.points.resize(cloud_in.points.size());
  }
  index.resize(cloud_in.points.size());
  if (cloud_in.is_dense) {
    if (&cloud_in != &cloud_out) cloud_out = cloud_in;
    for (std::size_t j = 0; j < cloud_out.points.size(); ++j) index[j] = static_cast<int>(j);
    return;
  }
  std::size_t j = 0;
  for (std::size_t i = 0; i < cloud_in.points.size(); ++i) {
    if (!std::isfinite(cloud_in.points[i].x) || !std::isfinite(cloud_in.points[i].y) || !std::isfinite(cloud_in.points[i].z)) continue;
    cloud_out.points[j] = cloud_in.points[i];
    index[j] = static_cast<int>(i);
    j++;
  }
  if (j != cloud_in.points.size()) {
    cloud_out.points.resize(j);
    index.resize(j);
  }
  cloud_out.height = 1;
  cloud_out.width = static_cast<std::uint32_t>(j);
  cloud_out.is_dense = true;
}

}  // namespace pcl
