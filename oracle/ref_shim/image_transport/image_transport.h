// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).
// image_transport::ImageTransport / Publisher: VisualOdometry::init advertises three visualisation topics; what is published there is dropped.
#pragma once
#include <string>
#include <ros/ros.h>
#include <sensor_msgs/Image.h>

namespace image_transport {
class Publisher {
 public:
  template <class M> void publish(const M&) const {}
};
class ImageTransport {
 public:
  explicit ImageTransport(const ros::NodeHandle&) {}
  Publisher advertise(const std::string&, unsigned) { return Publisher(); }
};
}  // namespace image_transport
