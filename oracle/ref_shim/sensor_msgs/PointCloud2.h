// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).
// sensor_msgs::PointCloud2: header.stamp / header.frame_id only (scan_registration.cpp:453-493 assigns them and publishes into a no-op).
#pragma once
#include <string>
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
};
}  // namespace sensor_msgs
