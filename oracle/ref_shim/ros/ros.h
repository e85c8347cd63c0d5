// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).
// roscpp, reduced to what the reference's classes touch:
//  * ros::param::get(name, value) — the parameter server is a map the harness fills (ros::param::shim_store()); like roscpp it returns
//    false and leaves `value` untouched when the name is unknown, and converts a stored number to the requested type;
//  * NodeHandle / Publisher — advertise(topic) hands out a Publisher bound to the topic; publish(msg) keeps a copy of the LAST message per
//    topic in ros::shim_topics(), where the harness reads it back (ros::shim_last<M>(topic)); Time — always zero; Duration — a number;
//  * ROS_INFO / ROS_WARN / ROS_ERROR / ROS_DEBUG — no-ops; ROS_BREAK — aborts, as ros/assert.h does.
// No math header is included and no math function is declared here on purpose: see tf/LinearMath/Scalar.h.
#pragma once
#include <cstdlib>
#include <map>
#include <memory>
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
  Time() {}
  explicit Time(double s) : sec(s) {}
  static Time now() { return Time(); }
  double toSec() const { return sec; }
};
struct Duration {
  double sec = 0.0;
  Duration() {}
  explicit Duration(double s) : sec(s) {}
};

inline std::map<std::string, std::shared_ptr<const void>>& shim_topics() { static std::map<std::string, std::shared_ptr<const void>> m; return m; }
// the last message published on `topic`, or null; M must be the type that was published there
template <class M> inline const M* shim_last(const std::string& topic) {
  auto it = shim_topics().find(topic);
  return it == shim_topics().end() ? nullptr : static_cast<const M*>(it->second.get());
}

class Publisher {
 public:
  Publisher() {}
  explicit Publisher(const std::string& topic) : topic_(topic) {}
  template <class M> void publish(const M& m) const { shim_topics()[topic_] = std::make_shared<const M>(m); }

 private:
  std::string topic_;
};

class Subscriber {};

class NodeHandle {
 public:
  NodeHandle() {}
  explicit NodeHandle(const std::string&) {}
  template <class M> Publisher advertise(const std::string& topic, unsigned) { return Publisher(topic); }
};

}  // namespace ros

#define ROS_INFO(...) ((void)0)
#define ROS_WARN(...) ((void)0)
#define ROS_ERROR(...) ((void)0)
#define ROS_DEBUG(...) ((void)0)
#define ROS_BREAK() std::abort()
