// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text; functional).
//
// pcl::KdTreeFLANN as laser_odometry.cpp:269,356,525-526 and laser_mapping.cpp:452-453,477,543 drive it: setInputCloud, then
// nearestKSearch(point, k, indices, squared distances) — exact search, f32 distances as flann::L2_Simple<float> sums them, ascending.
// The search itself is DELEGATED to the oracle's restatement (orc::KdTree, oracle/orc_pcl.cpp, linked into the reference library):
// pinning FLANN is not the aim.  Ties on equal distance resolve to the lowest index, the project's canonical rule (DESIGN.md section 2,
// branch table).  As in PCL 1.10, k is clipped to the number of points and both vectors are resized to it — so a search in an EMPTY
// cloud leaves them empty, and the reference's `pointSearchSqDis[0]` behind it would be undefined behaviour: the harness does not let
// it come to that (ref_loam_harness.cpp).
#pragma once
#include <vector>
#include "../../../orc_pcl.h"   // oracle/orc_pcl.h
#include <pcl/point_cloud.h>

namespace pcl {
template <class PointT>
class KdTreeFLANN {
 public:
  typedef boost::shared_ptr<KdTreeFLANN<PointT>> Ptr;
  void setInputCloud(const typename PointCloud<PointT>::ConstPtr& cloud) {
    pts_.resize(cloud->points.size());
    for (std::size_t i = 0; i < pts_.size(); i++) {
      const PointT& p = cloud->points[i];
      pts_[i].x = p.x; pts_[i].y = p.y; pts_[i].z = p.z; pts_[i].intensity = p.intensity;
    }
    tree_.build(pts_);
  }
  int nearestKSearch(const PointT& point, int k, std::vector<int>& k_indices, std::vector<float>& k_sqr_distances) const {
    if (k > static_cast<int>(pts_.size())) k = static_cast<int>(pts_.size());
    k_indices.resize(k);
    k_sqr_distances.resize(k);
    if (k == 0) return 0;
    const float q[3] = {point.x, point.y, point.z};
    return tree_.knn(q, k, k_indices.data(), k_sqr_distances.data());
  }

 private:
  orc::Cloud pts_;
  orc::KdTree tree_;
};
}  // namespace pcl
