// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).  Included by vloam_tf.h; nothing of it is used by the files built here.
#pragma once
#include <geometry_msgs/TransformStamped.h>
