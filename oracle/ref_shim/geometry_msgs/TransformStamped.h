// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).  Members of VloamTF that the files built here never touch.
#pragma once
#include <sensor_msgs/PointCloud2.h>
namespace geometry_msgs {
struct TransformStamped {
  std_msgs::Header header;
};
}  // namespace geometry_msgs
