"""-m gpu: the published clouds through the C++ class surface (include/vloam_hip/compat.hpp): Session(device, cfg, limits),
LaserMapping::publishedMap() and registeredCloud() against the C getters, and their pull-style behaviour on a default session."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROBE = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include "vloam_hip/compat.hpp"
static bool same(const vloam::Cloud& a, const std::vector<float>& b) {
  return a.size() * 4 == b.size() && (a.empty() || std::memcmp(&a[0].x, b.data(), b.size() * sizeof(float)) == 0);
}
static bool same(const vloam::Cloud& a, const vloam::Cloud& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(&a[0].x, &b[0].x, a.size() * sizeof(vloam::PointXYZI)) == 0);
}
static void sweep(std::FILE* f, int n_pts, vloam::ScanRegistration& sr, vloam::LaserOdometry& lo, vloam::LaserMapping& lm) {
  vloam::Cloud in((size_t)n_pts);
  if (std::fread(in.data(), sizeof(vloam::PointXYZI), (size_t)n_pts, f) != (size_t)n_pts) std::exit(2);
  sr.reset(); lm.reset();
  sr.input(in);
  vloam::Cloud full, sharp, lessSharp, flat, lessFlat;
  sr.output(full, sharp, lessSharp, flat, lessFlat);
  lo.input(full, sharp, lessSharp, flat, lessFlat);
  lo.solveLO();
  vloam::Quaterniond q; vloam::Vector3d t; vloam::Cloud cornerLast, surfLast, fullRes; bool skip_frame = false;
  lo.output(q, t, cornerLast, surfLast, fullRes, skip_frame);
  lm.input(cornerLast, surfLast, fullRes, q, t, skip_frame);
  lm.solveMapping();
}
int main(int argc, char** argv) {
  const int n_sweeps = std::atoi(argv[2]), n_pts = std::atoi(argv[3]);
  std::FILE* f = std::fopen(argv[1], "rb");
  vloam_config cfg; vloam_default_config(&cfg);
  {
    vloam_limits lim; vloam_default_limits(&lim);
    lim.map_pub_number = 2; lim.publish_registered_cloud = 1;
    auto session = std::make_shared<vloam::Session>(0, &cfg, lim);
    vloam::ScanRegistration sr(session); vloam::LaserOdometry lo(session); vloam::LaserMapping lm(session);
    for (int k = 0; k < n_sweeps; k++) {
      sweep(f, n_pts, sr, lo, lm);
      int frame = -2;
      const vloam::Cloud pm = lm.publishedMap(&frame), rc = lm.registeredCloud();
      long long n = 0; int fr = -2, nc = 0, fc = -2;
      if (vloam_get_published_map(session->get(), nullptr, 0, &n, &fr) != VLOAM_OK) return 3;
      std::vector<float> m((size_t)n * 4 + 4), c;
      if (vloam_get_published_map(session->get(), m.data(), n, &n, &fr) != VLOAM_OK) return 3;
      m.resize((size_t)n * 4);
      if (vloam_get_published_cloud(session->get(), nullptr, 0, &nc, &fc) != VLOAM_OK) return 3;
      c.resize((size_t)nc * 4 + 4);
      if (vloam_get_published_cloud(session->get(), c.data(), nc, &nc, &fc) != VLOAM_OK) return 3;
      c.resize((size_t)nc * 4);
      const bool publishing = (k + 1) % 2 == 0;
      std::printf("on %d %d %zu %d %zu %d %d %d %d\n", k, frame, pm.size(), fc, rc.size(), (int)(frame == fr && same(pm, m)), (int)same(rc, c),
                  publishing ? (int)same(pm, lm.map()) : -1, (int)same(rc, session->features(11)));
    }
  }
  {   // a session without the products: publishedMap() is map(), registeredCloud() is vloam_get_features(h, 11), as before
    std::rewind(f);
    auto session = std::make_shared<vloam::Session>(0, &cfg);
    vloam::ScanRegistration sr(session); vloam::LaserOdometry lo(session); vloam::LaserMapping lm(session);
    sweep(f, n_pts, sr, lo, lm);
    int frame = -2;
    const vloam::Cloud pm = lm.publishedMap(&frame);
    std::printf("off %d %zu %d %d\n", frame, pm.size(), (int)same(pm, lm.map()), (int)same(lm.registeredCloud(), session->features(11)));
  }
  return 0;
}
'''


def test_cpp_published_map_and_registered_cloud(tmp_path, sweeps):
    n, shape = 4, (64, 512)
    clouds = [sweeps(shape[0], shape[1], k) for k in range(n)]
    data = tmp_path / "sweeps.bin"
    np.stack(clouds).astype(np.float32).tofile(data)
    src, exe = tmp_path / "probe.cpp", tmp_path / "probe"
    src.write_text(PROBE)
    libdir = os.path.join(ROOT, "vloam-cmu-16833_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lvloam_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    out = [l.split() for l in subprocess.check_output([str(exe), str(data), str(n), str(clouds[0].shape[0])]).decode().strip().split("\n")]
    assert len(out) == n + 1
    for k in range(n):
        tag, kk, frame, n_map, f_cloud, n_cloud, map_same, cloud_same, map_live, cloud_live = out[k][0], *[int(v) for v in out[k][1:]]
        assert tag == "on" and kk == k
        assert frame == (-1 if k == 0 else (1 if k < 3 else 3)), out[k]      # map_pub_number = 2: sweeps 1 and 3 publish
        assert (n_map > 1000) == (k > 0) and f_cloud == k and n_cloud > 10000
        assert map_same == 1 and cloud_same == 1, "compat.hpp against the C getters, sweep %d" % k
        assert map_live == (1 if k % 2 == 1 else -1) and cloud_live == 1
    assert out[n][0] == "off" and [int(v) for v in out[n][1:]] == [-1, int(out[n][2]), 1, 1] and int(out[n][2]) > 1000
