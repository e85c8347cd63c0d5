// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text; functional).
//
// pcl::VoxelGrid<PointXYZI> as scan_registration.cpp:433-437 drives it: setInputCloud, setLeafSize, filter.  A second restatement of
// PCL 1.10 filters/include/pcl/filters/impl/voxel_grid.hpp applyFilter (downsample_all_data = true, min_points_per_voxel = 0, no
// field filter), sharing no code with oracle/orc_pcl.cpp: bounding box over the finite points,
// inverse leaf = 1 / leaf in f32, voxel index = floor(p * inv) - min box index, linear index with multipliers (1, dx, dx * dy),
// (index, point) pairs sorted by index, one centroid per run of equal indices (f32 sums of x, y, z, intensity divided by the count).
// It is still OUR reading of PCL, not PCL: VoxelGrid is cross-checked between two restatements, not pinned to the library.
//
// PCL sorts the pairs with std::sort, which leaves points of one voxel in an unspecified order, and the f32 sums then run in that
// order.  pcl::refshim::voxel_stable_order() selects between that literal call (false, the default) and the project's canonical
// order (true: input order within a voxel — what liborc.so and the device compute).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <utility>
#include <vector>
#include <pcl/filters/filter.h>
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

namespace pcl {
namespace refshim {
inline bool& voxel_stable_order() { static bool v = false; return v; }
// observation only: (points in, points out) of every filter() call since the harness last cleared it — the first two calls of
// LaserMapping::solveMapping (laser_mapping.cpp:432-440) are the corner and the surface stack, which live in locals there
// (opt-in: nothing is logged unless filter_log_on() is set — the harness sets it around LaserMapping::solveMapping only)
inline bool& filter_log_on() { static bool v = false; return v; }
inline void log_filter(int in, int out);
inline std::vector<std::pair<int, int>>& filter_log() { static std::vector<std::pair<int, int>> v; return v; }
inline void log_filter(int in, int out) { if (filter_log_on()) filter_log().push_back({in, out}); }
}  // namespace refshim

template <class PointT>
class VoxelGrid {
 public:
  void setInputCloud(const typename PointCloud<PointT>::ConstPtr& c) { input_ = c; }
  void setLeafSize(float lx, float ly, float lz) {
    leaf_[0] = lx; leaf_[1] = ly; leaf_[2] = lz;
    for (int a = 0; a < 3; a++) inv_[a] = 1.0f / leaf_[a];
  }
  void filter(PointCloud<PointT>& out) {
    out.header = input_->header;
    out.points.clear();
    out.height = 1;
    out.is_dense = true;
    const std::vector<PointT>& in = input_->points;
    if (in.empty()) { out.width = 0; refshim::log_filter(0, 0); return; }
    float lo[3], hi[3];
    for (int a = 0; a < 3; a++) { lo[a] = std::numeric_limits<float>::max(); hi[a] = -std::numeric_limits<float>::max(); }
    for (const PointT& p : in) {
      if (!input_->is_dense && (!std::isfinite(p.x) || !std::isfinite(p.y) || !std::isfinite(p.z))) continue;
      const float c[3] = {p.x, p.y, p.z};
      for (int a = 0; a < 3; a++) { lo[a] = std::min(lo[a], c[a]); hi[a] = std::max(hi[a], c[a]); }
    }
    std::int64_t cells = 1;
    for (int a = 0; a < 3; a++) cells *= static_cast<std::int64_t>((hi[a] - lo[a]) * inv_[a]) + 1;
    if (cells > static_cast<std::int64_t>(std::numeric_limits<std::int32_t>::max())) {  // PCL warns and returns the input
      out = *input_;
      refshim::log_filter(static_cast<int>(in.size()), static_cast<int>(out.points.size()));
      return;
    }
    int bmin[3], bdiv[3];
    for (int a = 0; a < 3; a++) {
      bmin[a] = static_cast<int>(std::floor(lo[a] * inv_[a]));
      bdiv[a] = static_cast<int>(std::floor(hi[a] * inv_[a])) - bmin[a] + 1;
    }
    const int mul[3] = {1, bdiv[0], bdiv[0] * bdiv[1]};
    struct Pair { unsigned voxel, point; };
    std::vector<Pair> pairs;
    pairs.reserve(in.size());
    for (unsigned i = 0; i < in.size(); i++) {
      const PointT& p = in[i];
      if (!input_->is_dense && (!std::isfinite(p.x) || !std::isfinite(p.y) || !std::isfinite(p.z))) continue;
      const int i0 = static_cast<int>(std::floor(p.x * inv_[0]) - static_cast<float>(bmin[0]));
      const int i1 = static_cast<int>(std::floor(p.y * inv_[1]) - static_cast<float>(bmin[1]));
      const int i2 = static_cast<int>(std::floor(p.z * inv_[2]) - static_cast<float>(bmin[2]));
      pairs.push_back({static_cast<unsigned>(i0 * mul[0] + i1 * mul[1] + i2 * mul[2]), i});
    }
    auto by_voxel = [](const Pair& a, const Pair& b) { return a.voxel < b.voxel; };
    if (refshim::voxel_stable_order()) std::stable_sort(pairs.begin(), pairs.end(), by_voxel);
    else std::sort(pairs.begin(), pairs.end(), by_voxel);
    for (std::size_t first = 0; first < pairs.size();) {
      std::size_t last = first;
      float sx = 0.f, sy = 0.f, sz = 0.f, si = 0.f;
      while (last < pairs.size() && pairs[last].voxel == pairs[first].voxel) {
        const PointT& p = in[pairs[last].point];
        sx += p.x; sy += p.y; sz += p.z; si += p.intensity;
        ++last;
      }
      const float n = static_cast<float>(last - first);
      PointT c;
      c.x = sx / n; c.y = sy / n; c.z = sz / n; c.intensity = si / n;
      out.points.push_back(c);
      first = last;
    }
    out.width = static_cast<std::uint32_t>(out.points.size());
    refshim::log_filter(static_cast<int>(in.size()), static_cast<int>(out.points.size()));
  }

 private:
  typename PointCloud<PointT>::ConstPtr input_;
  float leaf_[3] = {0.f, 0.f, 0.f}, inv_[3] = {0.f, 0.f, 0.f};
};

}  // namespace pcl
