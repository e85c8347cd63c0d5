// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).
// tf2_eigen: vloam_tf.h includes it for the Eigen types of its Isometry3f members; nothing compiled here converts between tf2 and Eigen.
#pragma once
#include <cstdio>
#include <memory>
#include <eigen3/Eigen/Dense>
