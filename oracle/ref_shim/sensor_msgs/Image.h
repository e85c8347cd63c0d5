// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).
// sensor_msgs::Image and the encoding name VisualOdometry::publish mentions; the harness never calls publish().
#pragma once
#include <memory>
#include <string>
#include <sensor_msgs/PointCloud2.h>

namespace sensor_msgs {
struct Image {
  std_msgs::Header header;
};
typedef std::shared_ptr<Image> ImagePtr;
namespace image_encodings {
const std::string RGB8 = "rgb8";
}
}  // namespace sensor_msgs
