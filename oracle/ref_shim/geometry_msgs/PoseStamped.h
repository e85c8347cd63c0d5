// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).
// geometry_msgs::Point / Quaternion / Pose / PoseStamped: plain data, as publish() of laser_odometry.cpp and laser_mapping.cpp fills them.
#pragma once
#include <sensor_msgs/PointCloud2.h>
namespace geometry_msgs {
struct Point { double x = 0, y = 0, z = 0; };
struct Quaternion { double x = 0, y = 0, z = 0, w = 1; };
struct Pose { Point position; Quaternion orientation; };
struct PoseWithCovariance { Pose pose; };
struct PoseStamped { std_msgs::Header header; Pose pose; };
}  // namespace geometry_msgs
