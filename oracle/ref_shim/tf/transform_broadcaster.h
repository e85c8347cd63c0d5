// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).
// tf/transform_broadcaster.h: includes what the real header includes first (see tf/LinearMath/Scalar.h); sendTransform sends nothing.
#pragma once
#include <tf/transform_datatypes.h>

namespace tf {
class TransformBroadcaster {
 public:
  void sendTransform(const StampedTransform&) {}
};
}  // namespace tf
