// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).
// nav_msgs::Odometry: header, child_frame_id and pose.pose, which publish() of laser_odometry.cpp:543-554 and laser_mapping.cpp:714-757
// fill; the harness reads them back from the stand-in publishers (ros/ros.h).
#pragma once
#include <memory>
#include <string>
#include <geometry_msgs/PoseStamped.h>
#include <sensor_msgs/PointCloud2.h>

namespace nav_msgs {
struct Odometry {
  typedef std::shared_ptr<const Odometry> ConstPtr;
  std_msgs::Header header;
  std::string child_frame_id;
  geometry_msgs::PoseWithCovariance pose;
};
}  // namespace nav_msgs
