// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text; functional, unlike tests/stubs/ which are syntax-only).
// Lets the host compiler build the reference's scan_registration.cpp / lidarFactor.hpp unmodified (oracle/Makefile, target `ref`).
//
// Restates PCL 1.10 common/include/pcl/impl/point_types.hpp: PointXYZ and PointXYZI as the reference uses them — public float members
// x, y, z (and intensity), default-constructed to zero.  PCL pads both to 16 / 32 bytes for SSE; no arithmetic of the reference
// depends on the padding, so it is left out (the harness copies points out field by field).
#pragma once
#include <cstdint>

namespace pcl {

struct PointXYZ {
  float x = 0.f, y = 0.f, z = 0.f;
  PointXYZ() = default;
  PointXYZ(float x_, float y_, float z_) : x(x_), y(y_), z(z_) {}
};

struct PointXYZI {
  float x = 0.f, y = 0.f, z = 0.f, intensity = 0.f;
};

}  // namespace pcl
