// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).
// visual_odometry.h includes this message_filters header and uses nothing of it (only a commented-out typedef).
#pragma once
