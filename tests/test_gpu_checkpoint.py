"""-m gpu: checkpoint and restore (vloam_checkpoint_size / _save / _load) — a sequence saved by one handle and resumed in another.

Handles are compared by bytes (.tobytes() of trajectory() and get_map(), same_cloud for clouds), as tests/test_gpu_map_growth.py compares a
growable handle with a fixed one.  The drives are that file's: 16 lines x 512 columns at 1.5 m/s with the VLP-16 launch parameters (about
1 340 corner and 2 100 surf stack points per sweep, some 800 / 600 new voxels), and the 64 x 512, speed 25.0, 140 m range drive of its raw-voxel
test.  One comparison against the oracle, at POSE_TOL = 1e-8, the bar of the existing mapping tests."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_laser_mapping import oracle_published_map, qdist, same_cloud

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RINGS, COLS, N = 16, 512, 6   # N sweeps before the checkpoint, N after
PARAMS = dict(minimum_range=0.3, mapping_line_resolution=0.2, mapping_plane_resolution=0.4, mapping_skip_frame=1)   # loam_velodyne_VLP_16.launch:3-13
POSE_TOL = 1e-8
MAX_POINTS = RINGS * COLS
LOG2 = 16


def handle(vl, **kw):
    return vl.Handle(0, **dict(dict(scan_line=RINGS, with_mapping=1, max_points=MAX_POINTS, max_frames=2 * N + 4, map_capacity_log2=LOG2, **PARAMS), **kw))


def header(data):
    """The fields of the checkpoint's header the tests look at (csrc/ckpt_format.h: CkptHeader)."""
    frames, mapped = struct.unpack_from("<ii", data, 88)
    n_rec = struct.unpack_from("<qq", data, 104)
    n_blk = struct.unpack_from("<qq", data, 120)
    n_deferred = struct.unpack_from("<ii", data, 136)
    map_off, map_bytes, map_count = struct.unpack_from("<qqq", data, 168 + 3 * 24)
    total, = struct.unpack_from("<q", data, 432)
    return dict(frames=frames, mapped=mapped, n_rec=n_rec, n_blk=n_blk, n_deferred=n_deferred, map_bytes=map_bytes, map_count=map_count, total=total)


def run(h, clouds, first, last):
    for k in range(first, last):
        h.process_scan(clouds[k])
    h.sync()


def state(h):
    return dict(tj=h.trajectory(), map=h.get_map(), features=[h.features(w) for w in (5, 6, 7, 8)], pose=h.odometry_pose(), frames=h.frame_count())


def assert_same_state(a, b, what):
    assert a["frames"] == b["frames"], what
    assert a["tj"].tobytes() == b["tj"].tobytes(), "%s: trajectory" % what
    assert a["map"].tobytes() == b["map"].tobytes(), "%s: map" % what
    for w, x, y in zip((5, 6, 7, 8), a["features"], b["features"]):
        assert same_cloud(x, y), "%s: features(%d)" % (what, w)
    assert all(np.array_equal(x, y) for x, y in zip(a["pose"], b["pose"])), "%s: odometry pose" % what


@pytest.fixture(scope="module")
def drive(vl, orc, synth):
    """The sweeps; the oracle's poses and final map; handle A (2N sweeps, uninterrupted); handle B: states after 1, 2 and N sweeps, its
    checkpoints after 1 and N sweeps, then continued to 2N without being destroyed.  Computed once, read-only."""
    import torch
    torch.zeros(1).cuda()   # torch brings a HIP runtime of its own: up before the library's first handle (tests/test_gpu_host_input.py)
    seq = synth.SynthSequence(n_rings=RINGS, n_azimuth=COLS, n_sweeps=2 * N + 1, speed=1.5)
    o = orc.Oracle(scan_line=RINGS, minimum_range=PARAMS["minimum_range"], line_res=PARAMS["mapping_line_resolution"],
                   plane_res=PARAMS["mapping_plane_resolution"], mapping_skip_frame=1, with_mapping=True)
    clouds, poses = [], []
    for k in range(2 * N):
        c = seq.sweep(k)
        assert o.process(c) == 0
        qw, tw, _, _ = o.lo_pose()
        qm, tm = o.map_published_pose()
        clouds.append(c)
        poses.append(np.concatenate([qw, tw, qm, tm]))
    a = handle(vl)
    run(a, clouds, 0, 2 * N)
    A = state(a)
    ckpt_A = a.checkpoint()
    a.close()
    b = handle(vl)
    run(b, clouds, 0, 1)
    ckpt_1 = b.checkpoint()
    run(b, clouds, 1, 2)
    B2 = state(b)
    run(b, clouds, 2, N)
    BN = state(b)
    ckpt_N = b.checkpoint()
    assert b.checkpoint() == ckpt_N, "two checkpoints of one state differ"
    run(b, clouds, N, 2 * N)
    B_end = state(b)
    b.close()
    return dict(clouds=clouds, poses=np.array(poses), oracle_map=oracle_published_map(o), A=A, ckpt_A=ckpt_A, ckpt_1=ckpt_1, B2=B2, BN=BN, ckpt_N=ckpt_N, B_end=B_end)


def resume(vl, drive, h, what):
    """The resume test on handle h, fresh: load the checkpoint of N sweeps, compare with B at the save, run the other N, compare with A."""
    h.restore(drive["ckpt_N"])
    assert_same_state(state(h), drive["BN"], "%s right after load" % what)
    run(h, drive["clouds"], N, 2 * N)
    assert_same_state(state(h), drive["A"], "%s after the other %d sweeps" % (what, N))


def test_resume_parity(vl, drive):
    assert_same_state(drive["B_end"], drive["A"], "the saving handle continued (save must change nothing)")
    c = handle(vl)
    resume(vl, drive, c, "fresh handle")
    tj, ref = c.trajectory(), drive["poses"]
    assert tj.shape == ref.shape
    for k in range(2 * N):   # one comparison against the oracle, the bar of the mapping tests
        assert qdist(tj[k, 0:4], ref[k, 0:4]) < POSE_TOL and np.linalg.norm(tj[k, 4:7] - ref[k, 4:7]) < POSE_TOL, k
        assert qdist(tj[k, 7:11], ref[k, 7:11]) < POSE_TOL and np.linalg.norm(tj[k, 11:14] - ref[k, 11:14]) < POSE_TOL, k
    assert same_cloud(c.get_map(), drive["oracle_map"]), "/laser_cloud_map of the resumed handle against the oracle"
    c.close()


def test_across_sizes(vl, drive):
    hd = header(drive["ckpt_N"])
    n_map = drive["BN"]["map"].shape[0]
    r = hd["n_rec"][0] + hd["n_rec"][1]
    print("checkpoint of %d sweeps: %d bytes, records %s, block keys %s, map points %d" % (N, len(drive["ckpt_N"]), hd["n_rec"], hd["n_blk"], n_map))
    assert hd["frames"] == N and hd["total"] == len(drive["ckpt_N"])
    assert n_map <= r <= 2 * n_map and hd["map_count"] == r and hd["map_bytes"] == 32 * r
    # a fixed handle with more slots than the saver had
    big = handle(vl, map_capacity_log2=LOG2 + 3)
    resume(vl, drive, big, "fixed handle of 2^%d slots" % (LOG2 + 3))
    # the same sweeps saved from a table of another size: the same size, and (the stream is in slot order) the same records
    big2 = handle(vl, map_capacity_log2=LOG2 + 3)
    run(big2, drive["clouds"], 0, N)
    other = big2.checkpoint()
    big2.close()
    big.close()
    assert len(other) == len(drive["ckpt_N"]) and header(other)["n_rec"] == hd["n_rec"]
    def recs(d):
        off = struct.unpack_from("<q", d, 168 + 3 * 24)[0]
        return sorted(d[o:o + 32] for o in range(off, off + 32 * r, 32))
    assert recs(other) == recs(drive["ckpt_N"]), "the same records, whatever the table size"
    # a growable handle that starts at 2^10: it must have grown
    g = handle(vl, map_capacity_log2=10, map_grow=1)
    g.restore(drive["ckpt_N"])
    lg = g.health()["map_log2"]
    assert all(0.6 * 2 ** lg[k] >= hd["n_rec"][k] and lg[k] > 10 for k in (0, 1)), lg
    assert_same_state(state(g), drive["BN"], "growable handle right after load")
    run(g, drive["clouds"], N, 2 * N)
    assert_same_state(state(g), drive["A"], "growable handle after the other sweeps")
    g.close()
    # a fixed handle that is too small for A's checkpoint: refused, still fresh, and a checkpoint that fits then resumes in it
    h1 = header(drive["ckpt_1"])
    need = 1.5 * max(max(h1["n_rec"]), 2 * max(h1["n_blk"])) / 0.6   # room for the checkpoint of one sweep and one more sweep (a sweep adds some 700 voxels to ~2 300)
    small_log2 = max(10, int(np.ceil(np.log2(need))))
    hA = header(drive["ckpt_A"])
    assert max(hA["n_rec"]) > 0.6 * 2 ** small_log2, (hA, small_log2)   # (the precondition of the refusal)
    t = handle(vl, map_capacity_log2=small_log2)
    with pytest.raises(vl.VloamError) as e:
        t.restore(drive["ckpt_A"])
    assert e.value.status == vl.ERR_CAPACITY and "live records" in str(e.value) and "2^%d" % small_log2 in str(e.value), str(e.value)
    assert t.frame_count() == 0
    t.restore(drive["ckpt_1"])
    run(t, drive["clouds"], 1, 2)
    assert_same_state(state(t), drive["B2"], "the small handle after a refused and a good load")
    t.close()
    # more frames than max_frames
    f = handle(vl, max_frames=N - 1)
    with pytest.raises(vl.VloamError) as e:
        f.restore(drive["ckpt_N"])
    assert e.value.status == vl.ERR_CAPACITY and "max_frames" in str(e.value)
    f.close()
    # a growable handle whose ceiling is too small
    gc = handle(vl, map_capacity_log2=10, map_grow=1, map_max_capacity_log2=11)
    with pytest.raises(vl.VloamError) as e:
        gc.restore(drive["ckpt_N"])
    assert e.value.status == vl.ERR_CAPACITY and "max_capacity_log2=11" in str(e.value)
    assert gc.health()["map_log2"] == (10, 10)
    gc.close()


def test_raw_voxels_tombstones_and_a_moved_window_inside_the_checkpoint(vl, synth, monkeypatch):
    """The recipe of test_gpu_map_growth.test_raw_voxels_across_a_growth.  The save point is the first sweep at which raw voxels exist
    (deferred > 0), records have been purged (purged > 0) and the window has moved: at 25 m/s over 20 sweeps the sensor crosses a cube border,
    so the centre cube — and with it the valid 5 x 5 x 3 block whose border turns voxels raw and whose advance re-filters them — is not where
    it was after the first sweep (the 21-cube grid itself rolls only after 350 m, outside any drive of a few seconds).  No such sweep: the test fails."""
    monkeypatch.setattr(synth, "MAX_RANGE", 140.0)
    n = 20   # (four sweeps more than that test: the centre cube moves at sweep 14, and a rest of the drive is to follow the checkpoint)
    seq = synth.SynthSequence(n_rings=64, n_azimuth=512, n_sweeps=n + 1, speed=25.0)
    clouds = [seq.sweep(k) for k in range(n)]
    mk = lambda: vl.Handle(0, with_mapping=1, map_capacity_log2=18, max_points=64 * 512)
    u = mk()
    save_at, centre0, seen = None, None, []
    for k in range(n):
        u.process_scan(clouds[k])
        if save_at is None:
            u.sync()
            mh, ms = u.map_health(), u.map_state()
            centre = tuple(int(x) for x in ms["centerCube"]) + tuple(int(x) for x in ms["cen"])
            centre0 = centre0 or centre
            seen.append((k, mh["deferred"], mh["purged"], centre))
            if k < n - 2 and sum(mh["deferred"]) > 0 and sum(mh["purged"]) > 0 and centre != centre0:
                save_at = k + 1
    assert save_at is not None, "no sweep with raw voxels, purged records and a moved window: %s" % seen
    u.sync()
    U = state(u)
    u.close()
    b = mk()
    run(b, clouds, 0, save_at)
    mh = b.map_health()
    assert sum(mh["deferred"]) > 0 and sum(mh["purged"]) > 0
    data = b.checkpoint()
    Bs = state(b)
    b.close()
    assert header(data)["n_deferred"] == mh["deferred"]
    for kw in (dict(map_capacity_log2=18), dict(map_capacity_log2=10, map_grow=1)):
        c = vl.Handle(0, with_mapping=1, max_points=64 * 512, **kw)
        c.restore(data)
        got = c.map_health()
        assert got["deferred"] == mh["deferred"] and got["purged"] == (0, 0), (got, mh)   # raw voxels re-appended, tombstones not carried over
        assert_same_state(state(c), Bs, "right after load %s" % kw)
        run(c, clouds, save_at, n)
        assert_same_state(state(c), U, "the rest of the drive %s" % kw)
        c.close()


def test_parameters(vl, drive, synth):
    clouds = drive["clouds"]
    # mapping_skip_frame = 2, the checkpoint on a skipped sweep (sweep index 4: (4 + 1) % 2 != 0)
    for kw, at, total in ((dict(mapping_skip_frame=2), 5, 8), (dict(with_mapping=0), 3, 6)):
        u = handle(vl, **kw)
        run(u, clouds, 0, total)
        b = handle(vl, **kw)
        run(b, clouds, 0, at)
        data, Bs = b.checkpoint(), state(b)
        b.close()
        c = handle(vl, **kw)
        c.restore(data)
        assert_same_state(state(c), Bs, "%s right after load" % kw)
        run(c, clouds, at, total)
        assert_same_state(state(c), state(u), "%s resumed" % kw)
        u.close()
        c.close()
    # a mismatch of each algorithmic parameter names the field
    for kw, field in ((dict(scan_line=32), "scan_line"), (dict(minimum_range=0.5), "minimum_range"), (dict(mapping_skip_frame=2), "mapping_skip_frame"),
                      (dict(mapping_line_resolution=0.4), "mapping_line_resolution"), (dict(mapping_plane_resolution=0.8), "mapping_plane_resolution"),
                      (dict(detach_VO_LO=0), "detach_VO_LO"), (dict(with_mapping=0), "with_mapping")):
        h = handle(vl, **kw)
        with pytest.raises(vl.VloamError) as e:
            h.restore(drive["ckpt_N"])
        assert e.value.status == vl.ERR_INVALID and field in str(e.value), (field, str(e.value))
        assert h.frame_count() == 0
        h.close()
    # the large stack tier on both sides; one side only is refused (the arrival stamps of raw points have another width there)
    seq = synth.SynthSequence(n_rings=64, n_azimuth=512, n_sweeps=7)
    big = [seq.sweep(k) for k in range(6)]
    mk = lambda **kw: vl.Handle(0, with_mapping=1, map_capacity_log2=18, max_points=64 * 512, **kw)
    u = mk(max_surf_stack_points=32768)
    run(u, big, 0, 6)
    b = mk(max_surf_stack_points=32768)
    run(b, big, 0, 3)
    data = b.checkpoint()
    b.close()
    c = mk(max_surf_stack_points=32768)
    c.restore(data)
    run(c, big, 3, 6)
    assert_same_state(state(c), state(u), "large stack tier")
    c.close()
    u.close()
    d = mk()
    with pytest.raises(vl.VloamError) as e:
        d.restore(data)
    assert e.value.status == vl.ERR_INVALID and "max_surf_stack_points" in str(e.value) and "large stack tier" in str(e.value)
    d.close()


def test_products(vl, drive):
    """map_pub_number = 4 and sweep_log on both sides: publications after the load happen at the frames of the uninterrupted run, with equal
    clouds; log rows before and after the checkpoint equal the uninterrupted handle's."""
    clouds = drive["clouds"]
    kw = dict(map_pub_number=4, sweep_log=1)
    u = handle(vl, **kw)
    pubs = []
    for k in range(2 * N):
        u.process_scan(clouds[k])
        u.sync()
        pubs.append(u.published_map())
    assert [f for _, f in pubs] == [-1] * 3 + [3] * 4 + [7] * 4 + [11]
    log_u = u.sweep_log()
    u.close()
    b = handle(vl, **kw)
    run(b, clouds, 0, N)
    data = b.checkpoint()
    b.close()
    c = handle(vl, **kw)
    c.restore(data)
    m, f = c.published_map()
    assert m.shape[0] == 0 and f == -1, "after load it is before the first publication"
    assert c.sweep_log().tobytes() == log_u[:N].tobytes(), "log rows of the restored sweeps"
    for k in range(N, 2 * N):
        c.process_scan(clouds[k])
        c.sync()
        m, f = c.published_map()
        if k < 7:
            assert f == -1
        else:
            assert f == pubs[k][1] and same_cloud(m, pubs[k][0]), "publication at sweep %d" % k
    assert c.sweep_log().tobytes() == log_u.tobytes(), "log rows before and after the checkpoint"
    c.close()
    # a loader without a log, and a saver without one: the run is the same, restored rows read frame == -1
    p = handle(vl, sweep_log=1)
    p.restore(drive["ckpt_N"])
    run(p, clouds, N, 2 * N)
    rows = p.sweep_log()
    assert list(rows["frame"]) == [-1] * N + list(range(N, 2 * N)) and rows[N:].tobytes() == log_u[N:].tobytes()
    assert p.trajectory().tobytes() == drive["A"]["tj"].tobytes()
    p.close()


def test_refusals(vl, drive, synth):
    L = vl.lib()
    clouds = drive["clouds"]
    # a batched handle
    hb = handle(vl, n_sessions=2)
    for call in (hb.checkpoint, lambda: hb.restore(drive["ckpt_N"])):
        with pytest.raises(vl.VloamError) as e:
            call()
        assert e.value.status == vl.ERR_INVALID and "n_sessions" in str(e.value)
    hb.close()
    # a handle after process_frame
    hf = handle(vl)
    hf.vo_set_calib(*synth.kitti_like_calib())
    hf.set_extrinsics(np.eye(4), np.eye(4))
    hf.process_frame(clouds[0], None, None)
    with pytest.raises(vl.VloamError) as e:
        hf.checkpoint()
    assert e.value.status == vl.ERR_ORDER and "VO" in str(e.value)
    hf.close()
    # a handle mid-stage
    hm = handle(vl)
    run(hm, clouds, 0, 2)
    hm.reset_frame()
    hm.scan_registration(clouds[2])
    with pytest.raises(vl.VloamError) as e:
        hm.checkpoint()
    assert e.value.status == vl.ERR_ORDER and "stage" in str(e.value)
    hm.laser_odometry()
    hm.laser_mapping()
    assert len(hm.checkpoint()) > 0   # ... and between two sweeps again it saves
    # a non-fresh handle on load
    with pytest.raises(vl.VloamError) as e:
        hm.restore(drive["ckpt_N"])
    assert e.value.status == vl.ERR_ORDER and "not fresh" in str(e.value)
    # cap too small: *bytes is still right and the buffer is untouched
    n, want = C.c_longlong(0), C.c_longlong(0)
    assert L.vloam_checkpoint_size(hm.h, C.byref(want)) == vl.VLOAM_OK and want.value > 448
    buf = C.create_string_buffer(b"\xa5" * want.value, want.value)
    assert L.vloam_checkpoint_save(hm.h, buf, C.c_longlong(want.value - 1), C.byref(n)) == vl.ERR_CAPACITY
    assert n.value == want.value and buf.raw == b"\xa5" * want.value
    assert L.vloam_checkpoint_save(hm.h, buf, C.c_longlong(want.value), C.byref(n)) == vl.VLOAM_OK and n.value == want.value
    hm.close()
    # a corrupted checkpoint is refused and leaves the handle fresh
    bad = bytearray(drive["ckpt_N"])
    bad[250] ^= 0x40   # the map section's byte count
    hc = handle(vl)
    with pytest.raises(vl.VloamError) as e:
        hc.restore(bytes(bad))
    assert e.value.status == vl.ERR_INVALID
    resume(vl, drive, hc, "after a refused corrupt load")
    hc.close()


def test_run_sequence_resume(tmp_path):
    """tools/run_sequence.py --save-checkpoint / --resume: the resumed run's result rows equal the tail of an uninterrupted run's."""
    tool = [sys.executable, os.path.join(ROOT, "tools", "run_sequence.py"), "--azimuth", "512"]
    ck = str(tmp_path / "seq.ckpt")
    r = subprocess.run(tool + ["--synthetic", "6", "--out", str(tmp_path / "full"), "--save-checkpoint", ck, "--at", "3"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run(tool + ["--synthetic", "6", "--out", str(tmp_path / "tail"), "--resume", ck], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for name in ("LO0.txt", "MO0.txt"):
        full = open(str(tmp_path / "full" / name)).read().splitlines()
        tail = open(str(tmp_path / "tail" / name)).read().splitlines()
        assert len(full) == 6 and len(tail) == 3 and tail == full[3:], name
