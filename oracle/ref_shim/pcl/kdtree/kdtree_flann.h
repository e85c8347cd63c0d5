// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).
// pcl::KdTreeFLANN: declaration only.  scan_registration.h and lidarFactor.hpp include the header without using the class; the files that
// search (laser_odometry.cpp, laser_mapping.cpp) are not built against this tree yet — a functional tree belongs here when they are.
#pragma once
#include <vector>
#include <pcl/point_cloud.h>

namespace pcl {
template <class PointT>
class KdTreeFLANN {
 public:
  typedef boost::shared_ptr<KdTreeFLANN<PointT>> Ptr;
  void setInputCloud(const typename PointCloud<PointT>::ConstPtr& cloud);
  int nearestKSearch(const PointT& point, int k, std::vector<int>& k_indices, std::vector<float>& k_sqr_distances) const;
};
}  // namespace pcl
