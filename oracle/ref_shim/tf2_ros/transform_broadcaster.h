// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).  VloamTF holds one by value; sendTransform broadcasts nothing here.
#pragma once
#include <geometry_msgs/TransformStamped.h>
namespace tf2_ros {
class TransformBroadcaster {
 public:
  void sendTransform(const geometry_msgs::TransformStamped&) {}
};
}  // namespace tf2_ros
