// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).
// tf/transform_datatypes.h: what matters to scan registration is what the real header drags in (tf/LinearMath/Scalar.h -> <math.h>, see
// there).  LaserMapping::publish (laser_mapping.cpp:767-776) also fills a tf::Transform for a broadcast that goes nowhere here: plain
// holders, no arithmetic.
#pragma once
#include <string>
#include <tf/LinearMath/Scalar.h>
#include <ros/ros.h>

namespace tf {
struct Vector3 {
  double v[3];
  Vector3(double x, double y, double z) : v{x, y, z} {}
};
class Quaternion {
 public:
  void setX(double x) { q_[0] = x; }
  void setY(double y) { q_[1] = y; }
  void setZ(double z) { q_[2] = z; }
  void setW(double w) { q_[3] = w; }
 private:
  double q_[4] = {0, 0, 0, 1};
};
class Transform {
 public:
  void setOrigin(const Vector3&) {}
  void setRotation(const Quaternion&) {}
};
struct StampedTransform {
  StampedTransform(const Transform&, const ros::Time&, const std::string&, const std::string&) {}
};
}  // namespace tf
