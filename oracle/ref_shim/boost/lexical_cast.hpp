// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).
// boost::lexical_cast<T>(string), which PointCloudUtil::loadTransformations parses the KITTI calibration files with.  The harness sets
// the calibration matrices directly and never calls that function; this is a stream extraction so that it would still work.
#pragma once
#include <sstream>
#include <string>
namespace boost {
template <class T> inline T lexical_cast(const std::string& s) {
  std::istringstream in(s);
  T v = T();
  in >> v;
  return v;
}
}  // namespace boost
