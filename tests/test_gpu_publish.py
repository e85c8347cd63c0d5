"""-m gpu: the clouds of LaserMapping::publish (laser_mapping.cpp:778-805) as products of the mapping stream — vloam_limits::map_pub_number,
max_published_map_points, publish_registered_cloud; vloam_get_published_map / _cloud / vloam_published_device_ptr.

/laser_cloud_map is ordered on the device (k_map_pub_*) behind the sweep that publishes it; the yardsticks are the CPU oracle's cube
clouds, vloam_get_map (device compaction + host sort) and, for the registered cloud, vloam_get_features(h, 11) of a default handle.  All
cloud comparisons are bit for bit: the order keys are unique and the publication adds no arithmetic.  (The recorded map of the reference
binary is compared by the rule of tests/test_gpu_ref_pinned_loam.py: there the POSES differ by round-off, whoever reads the map.)
"""
import os

import numpy as np
import pytest

import ref_cases

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
N_SWEEPS = 8
SHAPE = (64, 512)


def qdist(a, b):
    return min(np.linalg.norm(a - b), np.linalg.norm(a + b))


def oracle_published_map(o):
    """laserCloudMap of LaserMapping::publish (laser_mapping.cpp:778-793): for i in 0..4850: corner cube i, then surf cube i."""
    parts = []
    for c in range(21 * 21 * 11):
        for kind in (0, 1):
            p = o.map_cube(kind, c)
            if p.shape[0]:
                parts.append(p)
    return np.concatenate(parts) if parts else np.zeros((0, 4), np.float32)


def same_cloud(a, b):
    """x, y, z and intensity bit for bit in the same order."""
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a[:, :4]).view(np.uint32), np.ascontiguousarray(b[:, :4]).view(np.uint32))


def check_map_cloud(got, want, what):
    """tests/test_gpu_ref_pinned_loam.py: same points in the same order, intensities bit for bit; a coordinate is f32(q p + t) of f64 poses
    that agree to 1e-8, so it is the same float or its neighbour."""
    assert got.shape == want.shape and got.shape[0] > 100, "%s: %s vs %s points" % (what, got.shape, want.shape)
    g, w = np.ascontiguousarray(got[:, :4]), np.ascontiguousarray(want[:, :4])
    assert np.array_equal(g[:, 3].view(np.uint32), w[:, 3].view(np.uint32)), "%s intensities" % what
    ulp = np.abs(g[:, :3].view(np.int32).astype(np.int64) - w[:, :3].view(np.int32).astype(np.int64))
    print("%s: %d of %d coordinates not bit-equal (max %d ulp)" % (what, int(np.count_nonzero(ulp)), ulp.size, int(ulp.max())))
    assert ulp.max() <= 1 and np.mean(ulp == 0) > 0.999, what


@pytest.fixture(scope="module")
def oracle_run(orc, sweeps):
    """The 8 default 64 x 512 sweeps through the oracle, once: the published map after every sweep and the poses.  Read-only."""
    o = orc.Oracle(with_mapping=True)
    maps, poses = [], []
    for k in range(N_SWEEPS):
        assert o.process(sweeps(SHAPE[0], SHAPE[1], k)) == 0
        maps.append(oracle_published_map(o))
        qw, tw, _, _ = o.lo_pose()
        qm, tm = o.map_published_pose()
        poses.append(np.concatenate([qw, tw, qm, tm]))
    return maps, np.array(poses)


def check_poses(tj, poses):
    assert tj.shape == poses.shape
    for k in range(poses.shape[0]):
        assert qdist(tj[k, 0:4], poses[k, 0:4]) < 1e-8 and np.linalg.norm(tj[k, 4:7] - poses[k, 4:7]) < 1e-8, k
        assert qdist(tj[k, 7:11], poses[k, 7:11]) < 1e-8 and np.linalg.norm(tj[k, 11:14] - poses[k, 11:14]) < 1e-8, k


def test_every_sweep_publishes_the_oracles_map(vl, sweeps, oracle_run):
    maps, _ = oracle_run
    h = vl.Handle(0, with_mapping=1, map_pub_number=1)
    m, f = h.published_map()
    assert m.shape == (0, 4) and f == -1
    for k in range(N_SWEEPS):
        h.process_scan(sweeps(SHAPE[0], SHAPE[1], k))
        if k in (0, 3, 7):
            m, f = h.published_map()
            assert f == k and m.shape[0] > 1000
            assert same_cloud(m, maps[k]), "published map after sweep %d against the oracle" % k
            assert same_cloud(m, h.get_map()), "published map after sweep %d against vloam_get_map" % k
            p, n, fp = h.published_device_ptr(0)
            assert p and n == m.shape[0] and fp == k
    with pytest.raises(vl.VloamError) as e:    # the other product is off on this handle
        h.published_cloud()
    assert e.value.status == vl.ERR_ORDER
    h.close()


def test_a_publication_is_a_snapshot_of_its_sweep(vl, sweeps, oracle_run):
    """8 sweeps enqueued back to back, map_pub_number = 3: sweeps 2 and 5 publish; read after sweep 7 the product is the map after sweep 5."""
    maps, poses = oracle_run
    h = vl.Handle(0, with_mapping=1, map_pub_number=3)
    for k in range(N_SWEEPS):
        h.process_scan(sweeps(SHAPE[0], SHAPE[1], k))
    m, f = h.published_map()
    assert f == 5
    assert same_cloud(m, maps[5]) and not same_cloud(m, maps[7])
    check_poses(h.trajectory(), poses)
    h.close()


def test_skipped_sweeps_leave_the_last_publication_current(vl, orc, sweeps):
    """mapping_skip_frame = 2, map_pub_number = 4: sweeps 1, 3, 5, 7 are mapped (frameCount 1..4), (frameCount * 2) % 4 == 0 at sweeps 3 and 7."""
    h = vl.Handle(0, with_mapping=1, mapping_skip_frame=2, map_pub_number=4)
    o = orc.Oracle(with_mapping=True, mapping_skip_frame=2)
    seen = []
    for k in range(N_SWEEPS):
        c = sweeps(SHAPE[0], SHAPE[1], k)
        h.process_scan(c)
        assert o.process(c) == 0
        m, f = h.published_map()
        seen.append(f)
        if k in (3, 7):
            assert same_cloud(m, oracle_published_map(o)) and m.shape[0] > 1000, k
            at = m
        if k == 5:   # mapped, but not a publishing sweep: still sweep 3's map, which the live map has left behind
            assert f == 3 and same_cloud(m, at) and not same_cloud(m, h.get_map())
    assert seen == [-1, -1, -1, 3, 3, 3, 3, 7]
    h.close()


def test_raw_tails_beyond_the_valid_block(vl, orc, synth, monkeypatch):
    """The input of test_returns_beyond_the_valid_block (ranges up to 140 m: un-merged raw points behind the voxel-ordered part of a cube)."""
    monkeypatch.setattr(synth, "MAX_RANGE", 140.0)
    n = 16
    seq = synth.SynthSequence(n_rings=64, n_azimuth=512, n_sweeps=n + 1, speed=25.0)
    h = vl.Handle(0, with_mapping=1, map_pub_number=1)
    o = orc.Oracle(with_mapping=True)
    seen = 0
    for k in range(n):
        c = seq.sweep(k)
        h.process_scan(c)
        o.process(c)
        if k in (2, 8, 15):
            m, f = h.published_map()
            assert f == k and same_cloud(m, oracle_published_map(o)), "published map after sweep %d" % k
            h.sync()
            seen = max(seen, sum(h.map_health()["deferred"]))
    assert seen > 0, "the sequence must reach cubes outside the valid block"
    h.close()


def test_window_roll(vl, synth):
    """The drive of test_long_run_with_grid_roll (175 sweeps, 3 m apart: the cube window rolls, voxels of cubes that left it are purged);
    175 = 5 * 35, so the last sweep publishes."""
    n = 175
    seq = synth.SynthSequence(n_rings=64, n_azimuth=256, n_sweeps=n, speed=30.0)
    h = vl.Handle(0, with_mapping=1, map_pub_number=35)
    for k in range(n):
        h.process_scan(seq.sweep(k))
    m, f = h.published_map()
    h.sync()
    assert f == n - 1 and m.shape[0] > 1000
    assert not np.array_equal(h.map_state()["cen"], [10, 10, 5]), "the window must have rolled"
    assert same_cloud(m, h.get_map())
    h.close()


@pytest.mark.parametrize("name", ["ref_map_16x256", "ref_map_64x128"])
def test_the_reference_binarys_recorded_map(vl, name):
    z = np.load(os.path.join(HERE, "golden", name + ".npz"))
    p = ref_cases.loam_golden_params(z)
    n = int(z["n_sweeps"])
    h = vl.Handle(0, scan_line=p["scan_line"], minimum_range=p["minimum_range"], mapping_line_resolution=p["line_res"], mapping_plane_resolution=p["plane_res"],
                  mapping_skip_frame=p["mapping_skip_frame"], detach_VO_LO=int(p["detach_vo_lo"]), with_mapping=1, map_pub_number=1)
    for k in range(n):
        if int(z["has_prior"]):
            h.set_lo_prior(z["prior_%d" % k][:4], z["prior_%d" % k][4:])
        h.process_scan(ref_cases.loam_golden_sweep(z, k))
    m, f = h.published_map()
    assert f == n - 1
    check_map_cloud(m, z["map_cloud"], "published /laser_cloud_map, " + name)
    h.close()


@pytest.mark.parametrize("skip", [1, 2])
def test_registered_cloud(vl, sweeps, skip):
    """published_cloud() after each of 6 (7) sweeps against features(11) of a default handle fed the same sweeps and synchronised; then one sweep stage
    by stage with an edited laserCloudFullRes handed to LaserMapping::input: the product is the edited cloud's registration."""
    n = 6 if skip == 1 else 7    # the stage-wise sweep behind them is a MAPPED one (LaserMapping::input keeps only the pose of a skipped sweep)
    h = vl.Handle(0, with_mapping=1, mapping_skip_frame=skip, publish_registered_cloud=1)
    d = vl.Handle(0, with_mapping=1, mapping_skip_frame=skip)
    c0, f0 = h.published_cloud()
    assert c0.shape == (0, 4) and f0 == -1
    for k in range(n):
        c = sweeps(SHAPE[0], SHAPE[1], k)
        h.process_scan(c)
        d.process_scan(c)
        got, f = h.published_cloud()
        d.sync()
        want = d.features(11)
        assert f == k and got.shape[0] > 10000
        assert same_cloud(got, want), "registered cloud of sweep %d" % k
    c = sweeps(SHAPE[0], SHAPE[1], n)
    edited = None
    for hd in (h, d):
        hd.reset_frame()
        hd.scan_registration(c)
        hd.laser_odometry()
        if edited is None:
            full = hd.features(0)
            edited = full[: full.shape[0] // 2].copy()
        hd.set_mapping_input(laserCloudFullRes=edited)
        hd.laser_mapping()
    got, f = h.published_cloud()
    want = d.features(11)
    assert f == n and got.shape[0] == want.shape[0] == edited.shape[0] and same_cloud(got, want)
    p, cnt, fp = h.published_device_ptr(1)
    assert p and cnt == edited.shape[0] and fp == n
    with pytest.raises(vl.VloamError) as e:
        h.published_map()
    assert e.value.status == vl.ERR_ORDER
    h.close()
    d.close()


def test_batched_sessions(vl, synth):
    """Two different sequences in one batched handle, both products on.  Per session the products equal the session's own pull-style reads
    bit for bit, and those of a single-sequence handle fed that sequence."""
    n, B = 4, 2
    seqs = []
    for b in range(B):
        s = synth.SynthSequence(n_rings=SHAPE[0], n_azimuth=SHAPE[1], n_sweeps=n + 1, seed_scene=1234 + 17 * b, seed_traj=42 + b, seed_noise=5678 + 1000 * b)
        seqs.append([s.sweep(k) for k in range(n)])
    hb = vl.Handle(0, n_sessions=B, with_mapping=1, map_pub_number=1, publish_registered_cloud=1)
    for k in range(n):
        hb.batch_process_scan([seqs[b][k] for b in range(B)])
    got = []
    for b in range(B):
        hb.select(b)
        got.append((hb.published_map(), hb.published_cloud()))
    for b in range(B):
        hs = vl.Handle(0, with_mapping=1, map_pub_number=1, publish_registered_cloud=1)
        for k in range(n):
            hs.process_scan(seqs[b][k])
        (mb, fm), (cb, fc) = got[b]
        (ms, fms), (cs, fcs) = hs.published_map(), hs.published_cloud()
        assert fm == fc == fms == fcs == n - 1 and mb.shape[0] > 1000 and cb.shape[0] > 10000
        hb.select(b)
        assert same_cloud(mb, hb.get_map()) and same_cloud(cb, hb.features(11)), "session %d against its own pull-style reads" % b
        for what, x, y in (("map", mb, ms), ("registered cloud", cb, cs)):
            assert x.shape == y.shape, (b, what)
            ulp = np.abs(np.ascontiguousarray(x[:, :3]).view(np.int32).astype(np.int64) - np.ascontiguousarray(y[:, :3]).view(np.int32).astype(np.int64))
            print("session %d %s: %d of %d coordinates not bit-equal to the single-sequence handle's (max %d ulp)" % (b, what, int(np.count_nonzero(ulp)), ulp.size, int(ulp.max())))
            assert same_cloud(x, y), "session %d %s against a single-sequence handle" % (b, what)
        hs.close()
    assert not same_cloud(got[0][0][0], got[1][0][0]), "the sessions are different sequences"
    hb.close()


def test_overflow_is_reported_and_harmless(vl, sweeps, oracle_run):
    maps, poses = oracle_run
    h = vl.Handle(0, with_mapping=1, map_pub_number=1, max_published_map_points=256)
    for k in range(N_SWEEPS):
        h.process_scan(sweeps(SHAPE[0], SHAPE[1], k))
    full = h.get_map()
    assert full.shape[0] > 256
    L = vl.lib()
    import ctypes as C
    buf = np.full((256, 4), -7.0, np.float32)
    n, f = C.c_longlong(0), C.c_int(-1)
    st = L.vloam_get_published_map(h.h, buf.ctypes.data_as(C.c_void_p), C.c_longlong(256), C.byref(n), C.byref(f))
    assert st == vl.ERR_CAPACITY and n.value == full.shape[0] and f.value == N_SWEEPS - 1
    assert str(full.shape[0]).encode() in L.vloam_last_error() and b"256" in L.vloam_last_error()
    assert np.all(buf == -7.0), "no partial cloud"
    h.sync()
    check_poses(h.trajectory(), poses)
    again = h.get_map()
    assert same_cloud(again, full) and same_cloud(again, maps[N_SWEEPS - 1])
    h.close()


def test_off_means_off(vl, sweeps):
    """A default handle: the getters say the product is off, no k_map_pub_* / k_map_register launch, and every other kernel is launched as
    often as on a handle with the products on."""
    counts = []
    for kw in (dict(), dict(map_pub_number=1, publish_registered_cloud=1)):
        h = vl.Handle(0, with_mapping=1, **kw)
        h.profile_kernel("*", 4096)
        for k in range(N_SWEEPS):
            h.process_scan(sweeps(SHAPE[0], SHAPE[1], k))
        h.sync()
        counts.append({name: c for name, (_, c) in h.profile_table().items()})
        if not kw:
            for getter in (h.published_map, h.published_cloud, lambda: h.published_device_ptr(0), lambda: h.published_device_ptr(1)):
                with pytest.raises(vl.VloamError) as e:
                    getter()
                assert e.value.status == vl.ERR_ORDER
        h.close()
    off, on = counts
    new = [k for k in on if k.startswith("k_map_pub_") or k == "k_map_register"]
    assert not any(k.startswith("k_map_pub_") for k in off) and off.get("k_map_register", 0) == 0
    assert sorted(new) == ["k_map_pub_count", "k_map_pub_rank", "k_map_pub_scan", "k_map_pub_scatter", "k_map_pub_sort", "k_map_register"]
    assert all(on[k] == N_SWEEPS for k in new)
    assert {k: c for k, c in on.items() if k not in new} == off


def test_run_sequence_writes_the_publications(tmp_path):
    """tools/run_sequence.py --map-pub-number 2 over 6 synthetic sweeps, mapping_skip_frame 1: map_<frame>.npy for sweeps 1, 3 and 5, the
    count in the per-frame JSON; each file grows on the one before (the map only gains points over these sweeps)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(HERE)
    out = tmp_path / "res"
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "run_sequence.py"), "--synthetic", "6", "--azimuth", "512", "--mapping-skip-frame", "1",
                        "--map-pub-number", "2", "--metrics", str(tmp_path / "frames.jsonl"), "--out", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(f for f in os.listdir(out) if f.startswith("map_")) == ["map_%06d.npy" % k for k in (1, 3, 5)]
    maps = [np.load(out / ("map_%06d.npy" % k)) for k in (1, 3, 5)]
    assert all(m.dtype == np.float32 and m.shape[1] == 4 for m in maps) and 1000 < maps[0].shape[0] < maps[1].shape[0] < maps[2].shape[0]
    recs = [json.loads(l) for l in open(tmp_path / "frames.jsonl")]
    assert [r_["published_map"]["frame"] for r_ in recs] == [-1, 1, 1, 3, 3, 5]
    assert [r_["published_map"]["points"] for r_ in recs] == [None, maps[0].shape[0], None, maps[1].shape[0], None, maps[2].shape[0]]
    assert not any(r_["published_map"]["overflow"] for r_ in recs)
