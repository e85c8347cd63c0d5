// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).
// sensor_msgs::CameraInfo: the R and P arrays VisualOdometry::setUpPointCloud copies.  The harness sets the calibration matrices of the
// two PointCloudUtil objects directly (setUpPointCloud also needs Eigen::Isometry3f, which is not restated).
#pragma once
#include <memory>
#include <sensor_msgs/PointCloud2.h>

namespace sensor_msgs {
struct CameraInfo {
  std_msgs::Header header;
  double K[9] = {0}, R[9] = {0}, P[12] = {0};
};
typedef std::shared_ptr<const CameraInfo> CameraInfoConstPtr;
}  // namespace sensor_msgs
