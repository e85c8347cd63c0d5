// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).
// sensor_msgs::PointCloud2: the header, plus the payload as plain floats (x, y, z, intensity per point) instead of a serialised byte
// blob — pcl::toROSMsg (pcl_conversions stand-in) copies the cloud in, and the harness reads a published cloud back from it.
// `appended` carries the sizes of the clouds that operator+= joined into the source cloud (pcl/point_cloud.h), in order: for
// /laser_cloud_map (laser_mapping.cpp:780-785) that is the point count of every cube, corner and surface alternating.
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>
#include <ros/ros.h>

namespace std_msgs {
struct Header {
  unsigned seq = 0;
  ros::Time stamp;
  std::string frame_id;
};
}  // namespace std_msgs

namespace sensor_msgs {
struct PointCloud2 {
  std_msgs::Header header;
  std::vector<float> xyzi;
  std::vector<std::uint32_t> appended;
};
typedef std::shared_ptr<const PointCloud2> PointCloud2ConstPtr;
}  // namespace sensor_msgs
