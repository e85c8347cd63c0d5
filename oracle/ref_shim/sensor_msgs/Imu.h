// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).
// sensor_msgs::Imu: included by scan_registration.h, never used.
#pragma once
#include <sensor_msgs/PointCloud2.h>

namespace sensor_msgs {
struct Imu {
  std_msgs::Header header;
};
}  // namespace sensor_msgs
