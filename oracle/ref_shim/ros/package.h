// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).
// ros::package::getPath: point_cloud_util.h / image_util.h include the header; only commented-out lines use it.
#pragma once
#include <string>
namespace ros {
namespace package {
inline std::string getPath(const std::string&) { return std::string(); }
}  // namespace package
}  // namespace ros
