// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).
// pcl::toROSMsg / pcl::fromROSMsg: no-ops.  Only ScanRegistration::publish (scan_registration.cpp:451-499) calls them, and the harness
// reads the clouds through ScanRegistration::output instead of through messages.
#pragma once
#include <pcl/point_cloud.h>
#include <sensor_msgs/PointCloud2.h>

namespace pcl {
template <class PointT> inline void toROSMsg(const PointCloud<PointT>&, sensor_msgs::PointCloud2&) {}
template <class PointT> inline void fromROSMsg(const sensor_msgs::PointCloud2&, PointCloud<PointT>&) {}
}  // namespace pcl
