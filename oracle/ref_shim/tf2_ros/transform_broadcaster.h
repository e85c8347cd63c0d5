// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).  VloamTF holds one by value; it broadcasts nothing here.
#pragma once
namespace tf2_ros {
class TransformBroadcaster {};
}  // namespace tf2_ros
