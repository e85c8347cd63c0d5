// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).
// tf/transform_datatypes.h: the reference's scan registration uses nothing of tf; what matters is what the real header drags in
// (tf/LinearMath/Scalar.h -> <math.h>, see there).
#pragma once
#include <tf/LinearMath/Scalar.h>
