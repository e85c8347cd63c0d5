"""-m gpu: map merge (vloam_map_merge / vloam_map_merge_device) — two clouds of another map and the transform between the maps, folded into
the voxel map of a live handle.

What is checked, against tests/map_merge_model.py (pinned to the CPU oracle's VoxelGrid by tests/test_map_merge_model.py) bit for bit: a merge
at the identity into a fresh handle is an import; the fold onto a live map under a transform, every result field, on a fixed and a growable
handle, host and device form, twice; raw voxels stay as they are and their points are counted; a dry run writes nothing and counts what the
applied call counts; a merge far from the trajectory leaves every later pose as it was; readers and a checkpoint see the merged map like any
other; every refusal leaves the handle usable, and an overflowing fixed table is reported like a sweep's.

The clouds keep away from every voxel and cube face after the transform (faces: tests/test_gpu_voxel_faces.py), so the model's f64 floor is
the device's key.  Checkpoints are compared as: every byte outside the map section, and the map section's 32-byte records as a sorted list — the
stream is in slot order (csrc/ckpt_format.h), and which of two colliding keys gets the earlier slot is the claim order of one launch, which
neither an import nor a merge fixes (tests/test_gpu_checkpoint.py compares records the same way)."""
import struct

import numpy as np
import pytest

import map_merge_model as mm
from test_gpu_localize import bits, same_record, staged_sweep
from test_gpu_map_import import merge_cloud
from voxel_key_model import CEN0

pytestmark = pytest.mark.gpu

RINGS, AZ = 16, 256
LEAF = (0.4, 0.8)
Q, T = mm.POSE
FIELDS = ("n_in", "n_new_points", "n_hit_points", "n_skipped_raw", "n_outside_window", "n_nonfinite", "n_new_voxels", "max_per_voxel")
NONE = np.zeros((0, 4), np.float32)


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings a HIP runtime of its own: up before this module's first handle (tests/test_gpu_host_input.py); the device form takes tensors."""
    import torch
    torch.zeros(1).cuda()


def handle(vl, **kw):
    return vl.Handle(0, **dict(dict(scan_line=RINGS, with_mapping=1, map_capacity_log2=16), **kw))


def ckpt_parts(data):
    """(everything but the map section, its records sorted)"""
    off, nbytes, _ = struct.unpack_from("<qqq", data, 168 + 3 * 24)
    return data[:off] + data[off + nbytes:], sorted(data[o:o + 32] for o in range(off, off + nbytes, 32))


def same_rows(a, b):
    return sorted(bits(r) for r in a) == sorted(bits(r) for r in b)


def check_result(res, want, dry=False):
    for k in (0, 1):
        for f in FIELDS:
            w = 0 if dry and f in ("n_new_voxels", "max_per_voxel") else want[k]["res"][f]
            assert int(res[f][k]) == w, "kind %d, %s: %d, the model has %d (%s)" % (k, f, int(res[f][k]), w, res)


def check_map(h, want):
    for k in (0, 1):
        got, m = h.get_map_kind(k), want[k]["cloud"]
        assert got.shape == m.shape, (k, got.shape, m.shape)
        bad = np.flatnonzero((got.view(np.uint32) != m.view(np.uint32)).any(axis=1))
        assert bad.size == 0, "kind %d: %d of %d map points differ from the model, first %s vs %s" % (k, bad.size, got.shape[0], got[bad[:1]], m[bad[:1]])


@pytest.fixture(scope="module")
def case():
    """Clouds A (imported first) and B (merged under (Q, T)) of both kinds, and the model's answers; computed once, read-only."""
    pairs = [mm.cloud_pair(21 + k, LEAF[k]) for k in (0, 1)]
    first = [mm.merge(NONE, pairs[k][0], LEAF[k]) for k in (0, 1)]
    want = [mm.merge(first[k]["cloud"], pairs[k][1], LEAF[k], q=Q, t=T) for k in (0, 1)]
    return dict(A=[p[0] for p in pairs], B=[p[1] for p in pairs], first=first, want=want)


def test_fresh_handle_equals_import(vl):
    clouds = [merge_cloud(11, LEAF[0]), merge_cloud(12, LEAF[1])]
    for kw in (dict(map_capacity_log2=16), dict(map_capacity_log2=12, map_grow=1)):
        a, b = handle(vl, **kw), handle(vl, **kw)
        ri = a.map_import(clouds[0], clouds[1])
        rm = b.map_merge(clouds[0], clouds[1])
        for k in (0, 1):
            assert bits(a.get_map_kind(k)) == bits(b.get_map_kind(k)) and a.get_map_kind(k).shape[0] > 4000, k
            assert rm["n_new_voxels"][k] == ri["n_voxels"][k] and rm["n_new_points"][k] == clouds[k].shape[0] - ri["n_outside_window"][k]
            assert rm["n_outside_window"][k] == ri["n_outside_window"][k] and rm["max_per_voxel"][k] == ri["max_per_voxel"][k] == 4097
            assert rm["n_hit_points"][k] == 0 and rm["n_skipped_raw"][k] == 0 and rm["n_in"][k] == clouds[k].shape[0]
        assert a.map_health() == b.map_health() and a.health()["map_log2"] == b.health()["map_log2"]
        assert all(bits(a.map_state()[k]) == bits(b.map_state()[k]) for k in a.map_state())
        ca, cb = ckpt_parts(a.checkpoint()), ckpt_parts(b.checkpoint())
        assert ca[0] == cb[0], "checkpoint outside the map section"
        assert ca[1] == cb[1], "checkpoint: the map's records"
        with pytest.raises(vl.VloamError) as e:   # from here on it is a handle that holds a map: no import over it
            b.map_import(clouds[0], None)
        assert e.value.status == vl.ERR_ORDER
        a.close()
        b.close()


def test_fold_onto_a_live_map(vl, case):
    import torch
    want = case["want"]
    for k in (0, 1):
        r = want[k]["res"]
        assert r["n_hit_points"] > 12000 and r["n_new_points"] > 4000 and r["n_outside_window"] == 300 and r["max_per_voxel"] == 4097
    runs = []
    for kw in (dict(map_capacity_log2=16), dict(map_capacity_log2=12, map_grow=1), dict(map_capacity_log2=16)):
        h = handle(vl, **kw)
        h.map_import(case["A"][0], case["A"][1])
        check_map(h, case["first"])
        before = h.map_state()
        res = h.map_merge(case["B"][0], case["B"][1], q=Q, t=T)
        check_result(res, want)
        check_map(h, want)
        assert all(bits(h.map_state()[k]) == bits(before[k]) for k in before) and h.frame_count() == 0
        st = h.map_health()
        assert st["keys"] == tuple(want[k]["cloud"].shape[0] for k in (0, 1)) and st["purged"] == (0, 0) and st["deferred"] == (0, 0)
        if "map_grow" in kw:
            assert min(h.health()["map_log2"]) >= 14   # 6 000 voxels do not fit 60 % of 2^12 slots
        h.sync()
        runs.append((bits(h.get_map()), {f: bits(res[f]) for f in FIELDS}))
        h.close()
    assert runs[0] == runs[1] == runs[2], "merges of the same arrays differ"
    # the device form: the same arrays with a handful of non-finite points in between, dropped and counted
    dev = [mm.with_nonfinite(case["B"][k]) for k in (0, 1)]
    dwant = [mm.merge(case["first"][k]["cloud"], dev[k], LEAF[k], q=Q, t=T) for k in (0, 1)]
    assert all(dwant[k]["res"]["n_nonfinite"] == 7 and bits(dwant[k]["cloud"]) == bits(want[k]["cloud"]) for k in (0, 1))
    h = handle(vl, map_capacity_log2=15)
    h.map_import(case["A"][0], case["A"][1])
    res = h.map_merge_device(torch.from_numpy(dev[0]).cuda(), torch.from_numpy(dev[1]).cuda(), q=Q, t=T)
    check_result(res, dwant)
    check_map(h, dwant)
    assert bits(h.get_map()) == runs[0][0]
    with pytest.raises(vl.VloamError) as e:   # the host form refuses what the device form drops
        h.map_merge(dev[0], None, q=Q, t=T)
    assert e.value.status == vl.ERR_INVALID and "not finite" in str(e.value)
    assert bits(h.get_map()) == runs[0][0]
    h.close()


def test_dry_run_writes_nothing(vl, case):
    import torch
    h = handle(vl)
    h.map_import(case["A"][0], case["A"][1])
    before = h.checkpoint()
    res = h.map_merge(case["B"][0], case["B"][1], q=Q, t=T, apply=False)
    check_result(res, case["want"], dry=True)
    res = h.map_merge_device(torch.from_numpy(case["B"][0]).cuda(), torch.from_numpy(case["B"][1]).cuda(), q=Q, t=T, apply=False)
    check_result(res, case["want"], dry=True)
    assert h.checkpoint() == before, "a dry run changed what a checkpoint holds"
    # ... and on a fresh handle not even the window is placed
    f = handle(vl)
    before = f.checkpoint()
    res = f.map_merge(case["A"][0], case["A"][1], apply=False)
    assert [int(v) for v in res["n_new_points"]] == [case["A"][k].shape[0] for k in (0, 1)] and f.checkpoint() == before
    f.map_import(case["A"][0], case["A"][1])   # still fresh
    for x in (h, f):
        x.sync()
        x.close()


def test_raw_voxels_are_left_alone(vl, synth, monkeypatch):
    """Ranges up to 140 m (the drive of test_gpu_laser_mapping.test_returns_beyond_the_valid_block: 64 x 512, 25 m/s — 16 rings select no
    feature that far out) leave un-merged raw points in cubes outside the valid 5 x 5 x 3 block.  Merging those very points (they lie in raw
    voxels by construction) changes no record."""
    monkeypatch.setattr(synth, "MAX_RANGE", 140.0)
    seq = synth.SynthSequence(n_rings=64, n_azimuth=512, n_sweeps=9, speed=25.0)
    h = vl.Handle(0, with_mapping=1, map_capacity_log2=17)
    for k in range(8):
        h.process_scan(seq.sweep(k))
        h.sync()
        if sum(h.map_health()["deferred"]) > 0:
            break
    assert sum(h.map_health()["deferred"]) > 0, "the drive left no raw voxel"

    def dump(kind):
        return h.debug_raw(2, 67 + kind, np.uint32, max_bytes=1 << 30).reshape(-1, 7).copy()
    before = [dump(k) for k in (0, 1)]
    deferred = h.map_health()["deferred"]
    clouds, n_raw = [], []
    for k in (0, 1):
        d = before[k]
        seq_no, count = d[:, 1] >> 24, d[:, 2]
        raw_pts = d[seq_no != 0][:, 3:7].copy().view(np.float32)
        own = d[(seq_no == 0) & (count == 1)][:, 3:7].copy().view(np.float32)   # merged map points as well: those voxels do fold
        fv = own[:, :3].astype(np.float64) / LEAF[k]
        fv = fv - np.floor(fv)
        own = own[(np.minimum(fv, 1.0 - fv) > 0.01).all(axis=1)][:50]           # (a centroid off its voxel's faces keys back into its voxel)
        assert raw_pts.shape[0] > 0 and own.shape[0] == 50
        clouds.append(np.concatenate([raw_pts[: raw_pts.shape[0] // 2], own, raw_pts[raw_pts.shape[0] // 2:]]))
        n_raw.append(raw_pts.shape[0])
    res = h.map_merge(clouds[0], clouds[1])
    for k in (0, 1):
        assert int(res["n_skipped_raw"][k]) == n_raw[k] and int(res["n_hit_points"][k]) == 50 and int(res["n_new_points"][k]) == 0, res
        assert int(res["n_new_voxels"][k]) == 0 and int(res["max_per_voxel"][k]) == 1
        # every record as it was: the raw voxels and their point records untouched, and a map point folded onto itself is (c + c) / 2 = c
        assert sorted(bits(r) for r in dump(k)) == sorted(bits(r) for r in before[k]), "kind %d: a record changed" % k
    assert h.map_health()["deferred"] == deferred
    h.process_scan(seq.sweep(k + 1))
    h.sync()
    h.close()


def far_cloud(seed, leaf):
    """~1 500 points 300 - 400 m from the origin along +x: inside the window (cubes up to 525 m), outside the valid block (125 m)"""
    rng = np.random.default_rng(seed)
    g = mm._voxels(rng, np.array([300.0, -30.0, -10.0]), np.array([400.0, 30.0, 10.0]), leaf, 500)
    pts = mm._with_intensity(rng, mm._fill(rng, g, rng.integers(1, 6, size=500), leaf))
    return pts[rng.permutation(pts.shape[0])]


def test_far_merge_does_not_disturb_and_checkpoints(vl, sweeps):
    clouds = [sweeps(RINGS, AZ, k) for k in range(12)]

    def run(h, first, last):
        for k in range(first, last):
            h.process_scan(clouds[k])
        h.sync()
    a, b = handle(vl), handle(vl)
    run(a, 0, 6)
    for k in range(6):
        b.process_scan(clouds[k])   # (no sync: the merge flushes the deferred host sweep itself)
    far = [far_cloud(41 + k, LEAF[k]) for k in (0, 1)]
    res = b.map_merge(far[0], far[1])
    want = [mm.merge(NONE, far[k], LEAF[k]) for k in (0, 1)]
    check_result(res, want)
    assert b.frame_count() == 6 and bits(b.trajectory()) == bits(a.trajectory())
    for k in (0, 1):
        assert same_rows(b.get_map_kind(k), np.concatenate([a.get_map_kind(k), want[k]["cloud"]])), k
    ckpt = b.checkpoint()
    run(b, 6, 9)
    w = handle(vl, map_capacity_log2=17)
    w.restore(ckpt)
    run(w, 6, 9)
    assert bits(w.trajectory()) == bits(b.trajectory()) and bits(w.get_map()) == bits(b.get_map()), "the restored handle after 3 sweeps"
    assert all(bits(w.map_state()[k]) == bits(b.map_state()[k]) for k in b.map_state())
    w.close()
    run(b, 9, 12)
    run(a, 6, 12)
    assert bits(b.trajectory()) == bits(a.trajectory()) and a.trajectory().shape == (12, 14), "a pose moved after a merge 300 m away"
    for k in (0, 1):
        assert same_rows(b.get_map_kind(k), np.concatenate([a.get_map_kind(k), want[k]["cloud"]])), k
    a.close()
    b.close()


def test_near_merge_is_consistent_for_readers(vl, case, sweeps):
    h = handle(vl)
    h.map_import(case["A"][0], case["A"][1])
    h.map_merge(case["B"][0], case["B"][1], q=Q, t=T)
    halves = [h.get_map_kind(k).copy() for k in (0, 1)]
    f = handle(vl, map_capacity_log2=17)
    r = f.map_import(halves[0], halves[1])
    assert list(r["center_cube"]) == list(CEN0) == list(h.map_state()["cen"])
    assert all(bits(f.get_map_kind(k)) == bits(halves[k]) for k in (0, 1))
    src = vl.Handle(0, scan_line=RINGS, with_mapping=0)
    src.scan_registration(sweeps(RINGS, AZ, 0))
    corner, surf = src.features(2).copy(), src.features(4).copy()
    src.close()
    q0, t0 = np.array([0.0, 0.0, 0.0, 1.0]), np.array([5.0, 3.0, 0.5])
    la, lb = (x.map_localize(corner, surf, q0, t0, pose_frame=1) for x in (h, f))
    assert same_record(la, lb), (la, lb)
    rng = np.random.default_rng(3)
    qp = np.concatenate([halves[0][::9, :3], halves[1][::7, :3]])[:400] + rng.uniform(-0.3, 0.3, size=(400, 3)).astype(np.float32)
    qa, qb = (x.map_query(qp, k=5, max_radius=1.5, kind=2) for x in (h, f))
    assert (qa[2] > 0).sum() > 300 and all(bits(x) == bits(y) for x, y in zip(qa, qb))
    for x in (h, f):
        staged_sweep(x, sweeps(RINGS, AZ, 0))
    with pytest.raises(vl.VloamError) as e:   # in the middle of a stage-wise sweep: refused, and the sweep goes on
        h.map_merge(case["B"][0], None)
    assert e.value.status == vl.ERR_ORDER and "stage-wise" in str(e.value)
    pa, pb = h.laser_mapping(), f.laser_mapping()
    assert bits(pa[0]) == bits(pb[0]) and bits(pa[1]) == bits(pb[1])
    for x in (h, f):
        x.sync()
        x.close()


def test_refusals_leave_the_handle_usable(vl, case, sweeps):
    A, B = case["A"], case["B"]
    h = handle(vl)
    h.map_import(A[0], A[1])
    before = bits(h.get_map())
    texts = []
    for kw in (dict(apply=2), dict(q=[0.0, 0.0, 0.0, 1.01]), dict(t=[0.0, np.inf, 0.0])):
        with pytest.raises(vl.VloamError) as e:
            h.map_merge(B[0], B[1], **kw)
        assert e.value.status == vl.ERR_INVALID
        texts.append(str(e.value))
    assert "apply" in texts[0] and "norm" in texts[1] and "not finite" in texts[2] and bits(h.get_map()) == before
    h.process_scan(sweeps(RINGS, AZ, 0))
    h.sync()
    h.close()
    g = vl.Handle(0, n_sessions=2, scan_line=RINGS, with_mapping=1, map_capacity_log2=14)
    with pytest.raises(vl.VloamError) as e:
        g.map_merge(B[0], B[1])
    assert e.value.status == vl.ERR_INVALID and "n_sessions" in str(e.value)
    g.batch_process_scan([sweeps(RINGS, AZ, 0), sweeps(RINGS, AZ, 1)])
    g.sync()
    g.close()
    n = vl.Handle(0, scan_line=RINGS, with_mapping=0)
    with pytest.raises(vl.VloamError) as e:
        n.map_merge(B[0], B[1])
    assert e.value.status == vl.ERR_ORDER and "with_mapping" in str(e.value)
    n.process_scan(sweeps(RINGS, AZ, 0))
    n.sync()
    n.close()
    # a fixed table of 2^10 slots: 4 000 new voxels pass 60 % -> reported, sticky, like a sweep that filled the table
    s = handle(vl, map_capacity_log2=10)
    with pytest.raises(vl.VloamError) as e:
        s.map_merge(A[0], None)
    assert e.value.status == vl.ERR_CAPACITY and "corner" in str(e.value) and "60 %" in str(e.value), str(e.value)
    with pytest.raises(vl.VloamError) as e:
        s.sync()
    assert e.value.status == vl.ERR_CAPACITY
    s.close()
