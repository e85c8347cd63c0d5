// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).
// nav_msgs::Odometry: included by scan_registration.h, never used there.
#pragma once
#include <sensor_msgs/PointCloud2.h>

namespace nav_msgs {
struct Odometry {
  std_msgs::Header header;
};
}  // namespace nav_msgs
