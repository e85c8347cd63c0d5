// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).
// THE include that decides the arithmetic of the scan-line binning.
//
// The real tf/LinearMath/Scalar.h (geometry/tf, ROS Noetic) starts with `#include <math.h>`.  Under libstdc++ that is the C++ wrapper
// <math.h>, which pulls std::atan, std::sqrt, ... — float overloads included — into the global namespace.  scan_registration.cpp:192
// calls the unqualified `atan(point.z / sqrt(...))` on floats: with <cmath> alone only the C library's ::atan(double) / ::sqrt(double)
// are visible there; with <math.h> the float overloads win.  The reference's translation unit reaches this header through
// <tf/transform_datatypes.h> (scan_registration.h:47-48), so this stand-in includes <math.h> for that reason — and adds NOTHING else:
// no using-declaration, no math function.  Which overload the call then picks is the compiler's finding.
// -DREF_SHIM_NO_MATH_H builds the counter-factual (libref_cmath_only.so) so that a test can size the assumption.
#pragma once
#ifndef REF_SHIM_NO_MATH_H
#include <math.h>
#endif
