// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).  VloamTF holds one by value; it broadcasts nothing here.
#pragma once
namespace tf2_ros {
class StaticTransformBroadcaster {};
}  // namespace tf2_ros
