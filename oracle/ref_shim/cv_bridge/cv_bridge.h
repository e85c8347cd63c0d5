// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).
// cv_bridge::CvImage as VisualOdometry::publish builds it; inert, the harness never calls publish().
#pragma once
#include <string>
#include <opencv4/opencv2/opencv.hpp>
#include <sensor_msgs/Image.h>

namespace cv_bridge {
struct CvImage {
  CvImage() {}
  CvImage(const std_msgs::Header&, const std::string&, const cv::Mat&) {}
  sensor_msgs::ImagePtr toImageMsg() const { return sensor_msgs::ImagePtr(); }
};
}  // namespace cv_bridge
