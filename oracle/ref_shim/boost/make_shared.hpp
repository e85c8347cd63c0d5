// REFERENCE-BUILD STAND-IN — see boost/shared_ptr.hpp.
#pragma once
#include "shared_ptr.hpp"
