// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).
// cv::eigen2cv, which VisualOdometry::solveRANSAC names; inert, never reached (see opencv2/opencv.hpp).
#pragma once
#include <opencv4/opencv2/opencv.hpp>
namespace cv {
template <class M> inline void eigen2cv(const M&, Mat&) {}
}  // namespace cv
