// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).  VloamTF holds shared pointers to these; they stay null here.
#pragma once
namespace tf2_ros {
class Buffer {};
class TransformListener {};
}  // namespace tf2_ros
