// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text; functional).
// tf2_ros::Buffer: lookupTransform(target, source, time, timeout) returns the transform the harness stored for that (target, source) pair
// with shim_set — no tree, no interpolation, no composition: VloamTF::processStaticTransform asks for four fixed pairs.  A pair that was
// never stored aborts (the real Buffer throws tf2::LookupException, which the reference does not catch either).  header.frame_id /
// child_frame_id come back as target / source, as from the real Buffer.  TransformListener listens to nothing.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <utility>
#include <geometry_msgs/TransformStamped.h>
#include <ros/ros.h>
namespace tf2_ros {
class Buffer {
 public:
  void shim_set(const std::string& target, const std::string& source, const geometry_msgs::Transform& t) { store_[std::make_pair(target, source)] = t; }
  geometry_msgs::TransformStamped lookupTransform(const std::string& target, const std::string& source, const ros::Time&, const ros::Duration&) const {
    auto it = store_.find(std::make_pair(target, source));
    if (it == store_.end()) { std::fprintf(stderr, "tf2_ros::Buffer stand-in: no transform %s <- %s\n", target.c_str(), source.c_str()); std::abort(); }
    geometry_msgs::TransformStamped out;
    out.header.frame_id = target;
    out.child_frame_id = source;
    out.transform = it->second;
    return out;
  }

 private:
  std::map<std::pair<std::string, std::string>, geometry_msgs::Transform> store_;
};
class TransformListener {
 public:
  explicit TransformListener(const Buffer&) {}
};
}  // namespace tf2_ros
