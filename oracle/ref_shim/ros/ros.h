// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).
// roscpp, reduced to what the reference's classes touch:
//  * ros::param::get(name, value) — the parameter server is a map the harness fills (ros::param::shim_store()); like roscpp it returns
//    false and leaves `value` untouched when the name is unknown, and converts a stored number to the requested type;
//  * NodeHandle / Publisher / Time — no-ops (nothing is published; the harness reads the objects' outputs directly);
//  * ROS_INFO / ROS_WARN / ROS_ERROR / ROS_DEBUG — no-ops; ROS_BREAK — aborts, as ros/assert.h does.
// No math header is included and no math function is declared here on purpose: see tf/LinearMath/Scalar.h.
#pragma once
#include <cstdlib>
#include <map>
#include <string>

namespace ros {

namespace param {
inline std::map<std::string, double>& shim_store() { static std::map<std::string, double> m; return m; }
inline bool get(const std::string& key, int& v) {
  auto it = shim_store().find(key);
  if (it == shim_store().end()) return false;
  v = static_cast<int>(it->second);
  return true;
}
inline bool get(const std::string& key, double& v) {
  auto it = shim_store().find(key);
  if (it == shim_store().end()) return false;
  v = it->second;
  return true;
}
inline bool get(const std::string& key, float& v) {
  auto it = shim_store().find(key);
  if (it == shim_store().end()) return false;
  v = static_cast<float>(it->second);
  return true;
}
inline bool get(const std::string& key, bool& v) {
  auto it = shim_store().find(key);
  if (it == shim_store().end()) return false;
  v = it->second != 0.0;
  return true;
}
}  // namespace param

struct Time {
  double sec = 0.0;
  static Time now() { return Time(); }
  double toSec() const { return sec; }
};

class Publisher {
 public:
  template <class M> void publish(const M&) const {}
};

class Subscriber {};

class NodeHandle {
 public:
  NodeHandle() {}
  explicit NodeHandle(const std::string&) {}
  template <class M> Publisher advertise(const std::string&, unsigned) { return Publisher(); }
};

}  // namespace ros

#define ROS_INFO(...) ((void)0)
#define ROS_WARN(...) ((void)0)
#define ROS_ERROR(...) ((void)0)
#define ROS_DEBUG(...) ((void)0)
#define ROS_BREAK() std::abort()
