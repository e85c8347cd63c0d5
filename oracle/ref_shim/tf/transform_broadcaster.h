// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).
// tf/transform_broadcaster.h: unused by scan registration; includes what the real header includes first (see tf/LinearMath/Scalar.h).
#pragma once
#include <tf/transform_datatypes.h>

namespace tf {
class TransformBroadcaster {};
}  // namespace tf
