// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).
// geometry_msgs::Vector3 / Transform / TransformStamped: plain data, as vloam_tf.cpp fills and reads them (header.frame_id, child_frame_id,
// transform.translation / rotation).
#pragma once
#include <string>
#include <geometry_msgs/PoseStamped.h>
#include <sensor_msgs/PointCloud2.h>
namespace geometry_msgs {
struct Vector3 { double x = 0, y = 0, z = 0; };
struct Transform { Vector3 translation; Quaternion rotation; };
struct TransformStamped {
  std_msgs::Header header;
  std::string child_frame_id;
  Transform transform;
};
}  // namespace geometry_msgs
