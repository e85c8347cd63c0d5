// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).  nav_msgs::Path: a header and the list of stamped poses.
#pragma once
#include <vector>
#include <geometry_msgs/PoseStamped.h>
namespace nav_msgs {
struct Path {
  std_msgs::Header header;
  std::vector<geometry_msgs::PoseStamped> poses;
};
}  // namespace nav_msgs
