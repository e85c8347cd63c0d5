// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text; functional).
//
// ceres::Jet<T, N> — the dual number of Ceres Solver 2.0 include/ceres/jet.h, restated: value a, N partials v, and the rules
//   f + g, f - g, -f, f * g = (fa ga, fa gv + fv ga), f / g = (fa / ga, (fv - (fa / ga) gv) / ga), mixed Jet / scalar forms,
//   sqrt: v / (2 sqrt a); sin: cos(a) v; cos: -sin(a) v; acos: -v / sqrt(1 - a^2); abs: f for a >= 0 else -f;
//   comparisons look at the value only.
// A second entry next to oracle/orc_ceres.h, sharing no code with it.  T may be double or long double.
#pragma once
#include <cmath>
#include <limits>
#include <eigen3/Eigen/Dense>

namespace ceres {

template <class T, int N>
struct Jet {
  T a;
  T v[N];
  Jet() : a(T(0)) { for (int i = 0; i < N; i++) v[i] = T(0); }
  explicit Jet(const T& value) : a(value) { for (int i = 0; i < N; i++) v[i] = T(0); }
  Jet(const T& value, int k) : a(value) { for (int i = 0; i < N; i++) v[i] = T(0); v[k] = T(1); }
  Jet& operator+=(const Jet& g) { a += g.a; for (int i = 0; i < N; i++) v[i] += g.v[i]; return *this; }
};

template <class T, int N> inline Jet<T, N> operator+(const Jet<T, N>& f) { return f; }
template <class T, int N> inline Jet<T, N> operator-(const Jet<T, N>& f) { Jet<T, N> h; h.a = -f.a; for (int i = 0; i < N; i++) h.v[i] = -f.v[i]; return h; }
template <class T, int N> inline Jet<T, N> operator+(const Jet<T, N>& f, const Jet<T, N>& g) { Jet<T, N> h; h.a = f.a + g.a; for (int i = 0; i < N; i++) h.v[i] = f.v[i] + g.v[i]; return h; }
template <class T, int N> inline Jet<T, N> operator-(const Jet<T, N>& f, const Jet<T, N>& g) { Jet<T, N> h; h.a = f.a - g.a; for (int i = 0; i < N; i++) h.v[i] = f.v[i] - g.v[i]; return h; }
template <class T, int N> inline Jet<T, N> operator*(const Jet<T, N>& f, const Jet<T, N>& g) { Jet<T, N> h; h.a = f.a * g.a; for (int i = 0; i < N; i++) h.v[i] = f.a * g.v[i] + f.v[i] * g.a; return h; }
template <class T, int N> inline Jet<T, N> operator/(const Jet<T, N>& f, const Jet<T, N>& g) {
  Jet<T, N> h;
  const T g_inv = T(1) / g.a;
  const T q = f.a * g_inv;
  h.a = q;
  for (int i = 0; i < N; i++) h.v[i] = (f.v[i] - q * g.v[i]) * g_inv;
  return h;
}
template <class T, int N> inline Jet<T, N> operator+(const Jet<T, N>& f, T s) { Jet<T, N> h = f; h.a = f.a + s; return h; }
template <class T, int N> inline Jet<T, N> operator+(T s, const Jet<T, N>& f) { Jet<T, N> h = f; h.a = s + f.a; return h; }
template <class T, int N> inline Jet<T, N> operator-(const Jet<T, N>& f, T s) { Jet<T, N> h = f; h.a = f.a - s; return h; }
template <class T, int N> inline Jet<T, N> operator-(T s, const Jet<T, N>& f) { Jet<T, N> h; h.a = s - f.a; for (int i = 0; i < N; i++) h.v[i] = -f.v[i]; return h; }
template <class T, int N> inline Jet<T, N> operator*(const Jet<T, N>& f, T s) { Jet<T, N> h; h.a = f.a * s; for (int i = 0; i < N; i++) h.v[i] = f.v[i] * s; return h; }
template <class T, int N> inline Jet<T, N> operator*(T s, const Jet<T, N>& f) { Jet<T, N> h; h.a = s * f.a; for (int i = 0; i < N; i++) h.v[i] = s * f.v[i]; return h; }
template <class T, int N> inline Jet<T, N> operator/(const Jet<T, N>& f, T s) { Jet<T, N> h; const T s_inv = T(1) / s; h.a = f.a * s_inv; for (int i = 0; i < N; i++) h.v[i] = f.v[i] * s_inv; return h; }
template <class T, int N> inline Jet<T, N> operator/(T s, const Jet<T, N>& g) { Jet<T, N> h; h.a = s / g.a; const T m = -s / (g.a * g.a); for (int i = 0; i < N; i++) h.v[i] = g.v[i] * m; return h; }

#define REF_SHIM_JET_CMP(op) \
  template <class T, int N> inline bool operator op(const Jet<T, N>& f, const Jet<T, N>& g) { return f.a op g.a; } \
  template <class T, int N> inline bool operator op(const Jet<T, N>& f, T s) { return f.a op s; } \
  template <class T, int N> inline bool operator op(T s, const Jet<T, N>& g) { return s op g.a; }
REF_SHIM_JET_CMP(<)
REF_SHIM_JET_CMP(<=)
REF_SHIM_JET_CMP(>)
REF_SHIM_JET_CMP(>=)
REF_SHIM_JET_CMP(==)
REF_SHIM_JET_CMP(!=)
#undef REF_SHIM_JET_CMP

template <class T, int N> inline Jet<T, N> abs(const Jet<T, N>& f) { return f.a < T(0) ? -f : f; }
template <class T, int N> inline Jet<T, N> sqrt(const Jet<T, N>& f) {
  Jet<T, N> h;
  h.a = std::sqrt(f.a);
  const T m = T(1) / (T(2) * h.a);
  for (int i = 0; i < N; i++) h.v[i] = f.v[i] * m;
  return h;
}
template <class T, int N> inline Jet<T, N> sin(const Jet<T, N>& f) { Jet<T, N> h; h.a = std::sin(f.a); const T m = std::cos(f.a); for (int i = 0; i < N; i++) h.v[i] = m * f.v[i]; return h; }
template <class T, int N> inline Jet<T, N> cos(const Jet<T, N>& f) { Jet<T, N> h; h.a = std::cos(f.a); const T m = -std::sin(f.a); for (int i = 0; i < N; i++) h.v[i] = m * f.v[i]; return h; }
template <class T, int N> inline Jet<T, N> acos(const Jet<T, N>& f) { Jet<T, N> h; h.a = std::acos(f.a); const T m = -T(1) / std::sqrt(T(1) - f.a * f.a); for (int i = 0; i < N; i++) h.v[i] = m * f.v[i]; return h; }

}  // namespace ceres

namespace Eigen {
// include/ceres/jet.h specialises NumTraits for Jet: epsilon() is the scalar's epsilon with zero partials
template <class T, int N>
struct NumTraits<ceres::Jet<T, N>> {
  static ceres::Jet<T, N> epsilon() { return ceres::Jet<T, N>(std::numeric_limits<T>::epsilon()); }
};
}  // namespace Eigen
