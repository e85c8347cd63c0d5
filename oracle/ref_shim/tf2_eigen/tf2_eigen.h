// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text; functional).
// tf2::transformToEigen as vloam_tf.cpp uses it (on a TransformStamped and on a Transform).  Restated from geometry2 (ROS Noetic)
// tf2_eigen.h: Eigen::Isometry3d(Eigen::Translation3d(t) * Eigen::Quaterniond(w, x, y, z)) — the linear part is
// Quaternion::toRotationMatrix() of the message's quaternion AS IT IS (Eigen does not normalise it), the translation is copied.  The
// arithmetic of toRotationMatrix and of cast<float>() is written at the top of eigen3/Eigen/Dense.
#pragma once
#include <cstdio>
#include <memory>
#include <eigen3/Eigen/Dense>
#include <geometry_msgs/TransformStamped.h>
namespace tf2 {
inline Eigen::Isometry3d transformToEigen(const geometry_msgs::Transform& t) {
  return Eigen::Isometry3d::refshim_from(t.rotation.w, t.rotation.x, t.rotation.y, t.rotation.z, t.translation.x, t.translation.y, t.translation.z);
}
inline Eigen::Isometry3d transformToEigen(const geometry_msgs::TransformStamped& t) { return transformToEigen(t.transform); }
}  // namespace tf2
