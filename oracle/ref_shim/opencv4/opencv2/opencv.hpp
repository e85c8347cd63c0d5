// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).
// <opencv4/opencv2/opencv.hpp>: scan_registration.h includes it and uses nothing of it.  Deliberately empty: in particular it does not
// include <math.h> (the real OpenCV core headers include <cmath>, which does not bring the float overloads into the global namespace).
#pragma once
