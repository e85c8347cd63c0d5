// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).
// boost::shared_ptr / boost::make_shared as PCL 1.10's PointCloud<T>::Ptr uses them (scan_registration.cpp:82-86, :316): ownership
// semantics only, which std::shared_ptr provides identically.
#pragma once
#include <memory>

namespace boost {
template <class T> using shared_ptr = std::shared_ptr<T>;
using std::make_shared;
}  // namespace boost
