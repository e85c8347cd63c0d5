// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text; functional).
//
// tf2::Vector3 / Quaternion / Matrix3x3 / Transform as laser_odometry.cpp:225-232, :563-571 and laser_mapping.cpp:728-755 use them
// through the reference's own vloam_tf.h.  Restated from geometry2 (ROS Noetic) tf2/LinearMath/{Matrix3x3,Transform}.h: a Transform is a
// 3 x 3 basis plus an origin, so setRotation() stores a MATRIX (s = 2 / |q|^2; 1 - (yy + zz), xy - wz, ... ) and getRotation() extracts a
// quaternion from it again (trace > 0: s = sqrt(trace + 1), w = s / 2, the off-diagonal differences times 0.5 / s; otherwise the
// largest diagonal element leads) — what the reference reads back from velo_last_VOT_velo_curr is therefore NOT bit for bit what was
// stored, and the harness hands the oracle the read-back values.  inverse() = (basis^T, basis^T * -origin); a * b = (basis_a basis_b,
// basis_a origin_b + origin_a).  Unlike tf2, a default-constructed Transform is the identity rather than uninitialised memory.
//
// For visual_odometry.cpp:272-280, :426-430 (tf2/LinearMath/Quaternion.h): getAngle() = 2 acos(w) with w clamped to [-1, 1] (tf2Acos);
// getAxis() = (x, y, z) / sqrt(1 - w^2), or (1, 0, 0) when 1 - w^2 < 10 DBL_EPSILON; setRotation(axis, angle) = (axis sin(angle / 2) /
// |axis|, cos(angle / 2)); getX() ... of Vector3 and Quaternion; the nine-scalar Matrix3x3 constructor and Transform::setBasis; the
// conversion to const double* through which Eigen::Quaterniond / Vector3d are built from them (visual_odometry.cpp:457-458).
//
// For vloam_tf.cpp: Transform(q, origin) builds the basis by setRotation(q); a *= b is origin += basis * b.origin, THEN basis *= b.basis
// (tf2's order: the origin is moved with the basis as it was before the product).
#pragma once
#include <cfloat>
#include <cmath>

namespace tf2 {

class Vector3 {
 public:
  Vector3() : v_{0, 0, 0} {}
  Vector3(double x, double y, double z) : v_{x, y, z} {}
  double x() const { return v_[0]; }
  double y() const { return v_[1]; }
  double z() const { return v_[2]; }
  double getX() const { return v_[0]; }
  double getY() const { return v_[1]; }
  double getZ() const { return v_[2]; }
  double length() const { return std::sqrt(dot(*this)); }
  operator const double*() const { return v_; }
  double dot(const Vector3& o) const { return v_[0] * o.v_[0] + v_[1] * o.v_[1] + v_[2] * o.v_[2]; }
  Vector3 operator-() const { return Vector3(-v_[0], -v_[1], -v_[2]); }
  Vector3 operator+(const Vector3& o) const { return Vector3(v_[0] + o.v_[0], v_[1] + o.v_[1], v_[2] + o.v_[2]); }
  double operator[](int i) const { return v_[i]; }

 private:
  double v_[3];
};

class Quaternion {
 public:
  Quaternion() : q_{0, 0, 0, 1} {}
  Quaternion(double x, double y, double z, double w) : q_{x, y, z, w} {}
  double x() const { return q_[0]; }
  double y() const { return q_[1]; }
  double z() const { return q_[2]; }
  double w() const { return q_[3]; }
  double getX() const { return q_[0]; }
  double getY() const { return q_[1]; }
  double getZ() const { return q_[2]; }
  double getW() const { return q_[3]; }
  operator const double*() const { return q_; }
  double length2() const { return q_[0] * q_[0] + q_[1] * q_[1] + q_[2] * q_[2] + q_[3] * q_[3]; }
  void setRotation(const Vector3& axis, double angle) {
    const double d = axis.length();
    const double s = std::sin(angle * 0.5) / d;
    q_[0] = axis.x() * s; q_[1] = axis.y() * s; q_[2] = axis.z() * s; q_[3] = std::cos(angle * 0.5);
  }
  double getAngle() const {
    double w = q_[3];
    if (w < -1.0) w = -1.0;
    if (w > 1.0) w = 1.0;
    return 2.0 * std::acos(w);
  }
  Vector3 getAxis() const {
    const double s_squared = 1.0 - std::pow(q_[3], 2.0);
    if (s_squared < 10.0 * DBL_EPSILON) return Vector3(1.0, 0.0, 0.0);
    const double s = std::sqrt(s_squared);
    return Vector3(q_[0] / s, q_[1] / s, q_[2] / s);
  }

 private:
  double q_[4];
};

class Matrix3x3 {
 public:
  Matrix3x3() { setIdentity(); }
  Matrix3x3(double xx, double xy, double xz, double yx, double yy, double yz, double zx, double zy, double zz) { setValue(xx, xy, xz, yx, yy, yz, zx, zy, zz); }
  void setIdentity() { r_[0] = Vector3(1, 0, 0); r_[1] = Vector3(0, 1, 0); r_[2] = Vector3(0, 0, 1); }
  void setValue(double xx, double xy, double xz, double yx, double yy, double yz, double zx, double zy, double zz) {
    r_[0] = Vector3(xx, xy, xz); r_[1] = Vector3(yx, yy, yz); r_[2] = Vector3(zx, zy, zz);
  }
  void setRotation(const Quaternion& q) {
    double d = q.length2();
    double s = 2.0 / d;
    double xs = q.x() * s, ys = q.y() * s, zs = q.z() * s;
    double wx = q.w() * xs, wy = q.w() * ys, wz = q.w() * zs;
    double xx = q.x() * xs, xy = q.x() * ys, xz = q.x() * zs;
    double yy = q.y() * ys, yz = q.y() * zs, zz = q.z() * zs;
    setValue(1.0 - (yy + zz), xy - wz, xz + wy, xy + wz, 1.0 - (xx + zz), yz - wx, xz - wy, yz + wx, 1.0 - (xx + yy));
  }
  void getRotation(Quaternion& q) const {
    double trace = r_[0].x() + r_[1].y() + r_[2].z();
    double temp[4];
    if (trace > 0.0) {
      double s = std::sqrt(trace + 1.0);
      temp[3] = s * 0.5;
      s = 0.5 / s;
      temp[0] = (r_[2].y() - r_[1].z()) * s;
      temp[1] = (r_[0].z() - r_[2].x()) * s;
      temp[2] = (r_[1].x() - r_[0].y()) * s;
    } else {
      int i = r_[0].x() < r_[1].y() ? (r_[1].y() < r_[2].z() ? 2 : 1) : (r_[0].x() < r_[2].z() ? 2 : 0);
      int j = (i + 1) % 3;
      int k = (i + 2) % 3;
      double s = std::sqrt(r_[i][i] - r_[j][j] - r_[k][k] + 1.0);
      temp[i] = s * 0.5;
      s = 0.5 / s;
      temp[3] = (r_[k][j] - r_[j][k]) * s;
      temp[j] = (r_[j][i] + r_[i][j]) * s;
      temp[k] = (r_[k][i] + r_[i][k]) * s;
    }
    q = Quaternion(temp[0], temp[1], temp[2], temp[3]);
  }
  const Vector3& operator[](int i) const { return r_[i]; }
  Matrix3x3 transpose() const {
    Matrix3x3 m;
    m.setValue(r_[0].x(), r_[1].x(), r_[2].x(), r_[0].y(), r_[1].y(), r_[2].y(), r_[0].z(), r_[1].z(), r_[2].z());
    return m;
  }
  Vector3 operator*(const Vector3& v) const { return Vector3(r_[0].dot(v), r_[1].dot(v), r_[2].dot(v)); }
  Matrix3x3 operator*(const Matrix3x3& o) const {
    Matrix3x3 t = o.transpose(), m;
    m.setValue(r_[0].dot(t[0]), r_[0].dot(t[1]), r_[0].dot(t[2]), r_[1].dot(t[0]), r_[1].dot(t[1]), r_[1].dot(t[2]), r_[2].dot(t[0]),
               r_[2].dot(t[1]), r_[2].dot(t[2]));
    return m;
  }

 private:
  Vector3 r_[3];
};

class Transform {
 public:
  Transform() {}
  Transform(const Matrix3x3& b, const Vector3& o) : basis_(b), origin_(o) {}
  Transform(const Quaternion& q, const Vector3& o) : origin_(o) { basis_.setRotation(q); }   // Matrix3x3(q) = setRotation(q)
  Transform& operator*=(const Transform& t) { origin_ = (*this)(t.origin_); basis_ = basis_ * t.basis_; return *this; }   // origin first, as tf2
  void setIdentity() { basis_.setIdentity(); origin_ = Vector3(0, 0, 0); }
  void setOrigin(const Vector3& o) { origin_ = o; }
  void setRotation(const Quaternion& q) { basis_.setRotation(q); }
  void setBasis(const Matrix3x3& b) { basis_ = b; }
  const Vector3& getOrigin() const { return origin_; }
  Quaternion getRotation() const { Quaternion q; basis_.getRotation(q); return q; }
  const Matrix3x3& getBasis() const { return basis_; }
  Vector3 operator()(const Vector3& x) const { return basis_ * x + origin_; }
  Transform inverse() const { Matrix3x3 inv = basis_.transpose(); return Transform(inv, inv * -origin_); }
  Transform operator*(const Transform& t) const { return Transform(basis_ * t.basis_, (*this)(t.origin_)); }

 private:
  Matrix3x3 basis_;
  Vector3 origin_;
};

}  // namespace tf2
