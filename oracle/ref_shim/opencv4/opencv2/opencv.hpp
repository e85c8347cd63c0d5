// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).
// <opencv4/opencv2/opencv.hpp>: scan_registration.h includes it and uses nothing of it; point_cloud_util.cpp, visual_odometry.cpp and
// image_util.h name the types and functions below.  INERT STUBS: cv::KeyPoint / DMatch / Point2f are plain data that the harness fills
// (VisualOdometry::keypoints, matches, keypoints_2f); everything else — Mat, the drawing and window calls, imread, CLAHE,
// findEssentialMat / recoverPose — does nothing and is never reached by what the harness calls (projectPointCloud, downsamplePointCloud,
// queryDepth, reset, solveNlsAll).  OpenCV itself is not pinned.
// Deliberately no <math.h> here (the real OpenCV core headers include <cmath>, which does not bring the float overloads into the global
// namespace): see tf/LinearMath/Scalar.h.
#pragma once
#include <memory>
#include <string>
#include <tuple>
#include <vector>

typedef unsigned char uchar;

namespace cv {

template <class T>
struct Point_ {
  T x, y;
  Point_() : x(0), y(0) {}
  Point_(T x_, T y_) : x(x_), y(y_) {}
};
typedef Point_<int> Point;
typedef Point_<float> Point2f;

struct Size { int width = 0, height = 0; };
struct Scalar {
  double val[4];
  Scalar(double a = 0, double b = 0, double c = 0, double d = 0) : val{a, b, c, d} {}
};

struct Mat {
  Size size() const { return Size(); }
  Mat clone() const { return Mat(); }
  Mat colRange(int, int) const { return Mat(); }
  int type() const { return 0; }
  template <class T> T at(int, int) const { return T(); }
};

struct KeyPoint {
  Point2f pt;
  float size = 0.f, angle = -1.f, response = 0.f;
  int octave = 0, class_id = -1;
};
struct DMatch {
  int queryIdx = -1, trainIdx = -1, imgIdx = -1;
  float distance = 0.f;
};

enum { IMREAD_GRAYSCALE = 0, COLOR_GRAY2BGR = 8, FILLED = -1, LINE_8 = 8, WINDOW_AUTOSIZE = 1, EVENT_LBUTTONDOWN = 1, LMEDS = 4, RANSAC = 8 };

inline Mat imread(const std::string&, int) { return Mat(); }
inline void cvtColor(const Mat&, Mat&, int) {}
inline void circle(Mat&, Point, int, const Scalar&, int, int) {}
inline void namedWindow(const std::string&, int) {}
inline void imshow(const std::string&, const Mat&) {}
inline int waitKey(int) { return -1; }
inline void setMouseCallback(const std::string&, void (*)(int, int, int, int, void*), void*) {}
inline Mat findEssentialMat(const std::vector<Point2f>&, const std::vector<Point2f>&, const Mat&, int, double, double) { return Mat(); }
inline int recoverPose(const Mat&, const std::vector<Point2f>&, const std::vector<Point2f>&, const Mat&, Mat&, Mat&, double) { return 0; }

template <class T> using Ptr = std::shared_ptr<T>;
struct CLAHE {
  void apply(const Mat&, Mat&) {}
};
inline Ptr<CLAHE> createCLAHE(double = 40.0) { return std::make_shared<CLAHE>(); }

}  // namespace cv
