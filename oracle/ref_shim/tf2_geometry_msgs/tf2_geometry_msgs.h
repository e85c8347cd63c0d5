// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text; functional).
// tf2::toMsg / tf2::fromMsg between tf2::Transform and geometry_msgs::Transform, as vloam_tf.cpp uses them.  Restated from geometry2 (ROS
// Noetic) tf2_geometry_msgs.h: toMsg copies the origin and getRotation() — the QUATERNION EXTRACTED FROM THE BASIS (Matrix3x3::getRotation,
// see tf2/LinearMath/Transform.h), so a NaN anywhere in the basis reaches rotation.x ... w through the trace; fromMsg builds
// tf2::Transform(tf2::Quaternion(x, y, z, w), tf2::Vector3(x, y, z)), i. e. the basis by Matrix3x3::setRotation (s = 2 / |q|^2: the message's
// quaternion need not be normalised).
#pragma once
#include <geometry_msgs/TransformStamped.h>
#include <tf2/LinearMath/Transform.h>
namespace tf2 {
inline geometry_msgs::Transform toMsg(const Transform& in) {
  geometry_msgs::Transform out;
  out.translation.x = in.getOrigin().x(); out.translation.y = in.getOrigin().y(); out.translation.z = in.getOrigin().z();
  const Quaternion q = in.getRotation();
  out.rotation.x = q.x(); out.rotation.y = q.y(); out.rotation.z = q.z(); out.rotation.w = q.w();
  return out;
}
inline void fromMsg(const geometry_msgs::Transform& in, Transform& out) {
  out = Transform(Quaternion(in.rotation.x, in.rotation.y, in.rotation.z, in.rotation.w), Vector3(in.translation.x, in.translation.y, in.translation.z));
}
}  // namespace tf2
