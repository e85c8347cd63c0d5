"""-m gpu: map clean-up (vloam_map_carve) against its NumPy statement (tests/carve_model.py), bit for bit, and what apply leaves behind.

The scene (tests/carve_scene.py; checked on the CPU oracle's map by tests/test_carve_scene.py): 16 x 256 synthetic sweeps, a phantom box of
about 200 returns 10 - 12 m ahead cast into sweeps 0 and 1 only, the map built from sweeps 0 - 4, the carve done with sweeps 3 and 4 under
their trajectory (map) poses, sweeps 5 and 6 driven afterwards.  The model runs on get_map_kind's points; no candidate is set aside: device
and model perform the same f32 operations, so the removed set and every counter are equal, not close."""
import ctypes as C

import numpy as np
import pytest

import carve_model as cm
import carve_scene as cs

pytestmark = pytest.mark.gpu

COUNTERS = ("examined", "in_view", "seen_through", "confirmed", "removed")


def handle(vl, **kw):
    return vl.Handle(0, scan_line=cs.RINGS, with_mapping=1, max_points=cs.MAX_POINTS, max_frames=16, **dict(cs.PARAMS, **kw))


def drive(h, sweeps, first, last):
    for k in range(first, last):
        h.process_scan(sweeps[k])
    h.sync()


@pytest.fixture(scope="module")
def scene(synth):
    import torch
    torch.zeros(1).cuda()   # torch brings a HIP runtime of its own: up before the library's first handle, as in tests/test_gpu_host_input.py
    return cs.build(synth)[0]


def carve_args(h, sweeps):
    tj = h.trajectory()
    poses = np.array([np.concatenate([tj[k, 7:11], tj[k, 11:14]]) for k in cs.CARVE_SWEEPS])
    return [sweeps[k] for k in cs.CARVE_SWEEPS], poses


def same_rows(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.fixture(scope="module")
def reference(vl, scene):
    """One dry run on a fixed handle next to the model's answer on its maps, shared by the tests below.  Read-only."""
    h = handle(vl)
    drive(h, scene, 0, cs.N_BUILD)
    maps = [h.get_map_kind(kind) for kind in (0, 1)]
    cs_, poses = carve_args(h, scene)
    removed, res = h.map_carve(cs_, poses, **cs.CARVE)
    after = [h.get_map_kind(kind) for kind in (0, 1)]
    health = h.map_health()
    h.close()
    model = [cm.carve(maps[kind], cs_, poses, **cs.CARVE) for kind in (0, 1)]
    return dict(maps=maps, after=after, removed=removed, res=res, model=model, poses=poses, health=health)


def test_dry_run_equals_the_model(reference):
    r = reference
    want = np.concatenate([r["maps"][kind][r["model"][kind][0]] for kind in (0, 1)])
    for kind in (0, 1):
        got = {k: int(r["res"][k][kind]) for k in COUNTERS}
        print("kind %d: device %s, model %s" % (kind, got, r["model"][kind][1]))
        assert got == r["model"][kind][1]
        assert int(r["res"]["skipped_raw"][kind]) == 0   # every return lies inside the valid block: no un-merged raw points (with them: tests/test_gpu_carve_raw.py)
        assert same_rows(r["maps"][kind], r["after"][kind]), "a dry run leaves the map as it was"
    assert r["res"]["n_removed_out"] == want.shape[0] == r["removed"].shape[0] > 0
    assert same_rows(cs.sorted_rows(r["removed"]), cs.sorted_rows(want))
    assert r["health"]["purged"] == (0, 0)


def test_the_phantom_leaves(reference):
    r = reference
    gone = {row.tobytes() for row in np.ascontiguousarray(r["removed"])}
    n_body = n_model = n_static = n_static_gone = 0
    for kind in (0, 1):
        pts, removed = r["maps"][kind], r["model"][kind][0]
        body = cs.in_phantom(pts) & (pts[:, 2] > cs.BOX[2] + 0.5)
        n_body, n_model = n_body + int(body.sum()), n_model + int((body & removed).sum())
        for row in np.ascontiguousarray(pts[body & removed]):
            assert row.tobytes() in gone
        n_static, n_static_gone = n_static + int((~cs.in_phantom(pts)).sum()), n_static_gone + int((~cs.in_phantom(pts) & removed).sum())
    print("phantom voxels above the ground: %d, removed %d; static voxels: %d, removed (false removals) %d" % (n_body, n_model, n_static, n_static_gone))
    assert n_body >= 20 and 2 * n_model >= n_body   # (tests/test_carve_scene.py: the rest has no return behind it)


@pytest.mark.parametrize("grow", [0, 1], ids=["fixed", "growable"])
def test_apply(vl, scene, reference, grow):
    h = handle(vl, **(dict(map_grow=1, map_capacity_log2=14) if grow else {}))
    drive(h, scene, 0, cs.N_BUILD)
    before = [h.get_map_kind(kind) for kind in (0, 1)]
    for kind in (0, 1):
        assert same_rows(before[kind], reference["maps"][kind])
    cs_, poses = carve_args(h, scene)
    hl0, mh0 = h.health(), h.map_health()
    removed, res = h.map_carve(cs_, poses, apply=True, **cs.CARVE)
    assert same_rows(cs.sorted_rows(removed), cs.sorted_rows(reference["removed"]))
    assert {k: res[k].tolist() for k in COUNTERS} == {k: reference["res"][k].tolist() for k in COUNTERS}
    after = [h.get_map_kind(kind) for kind in (0, 1)]
    gone = {row.tobytes() for row in np.ascontiguousarray(removed)}
    for kind in (0, 1):
        keep = np.array([row.tobytes() not in gone for row in np.ascontiguousarray(before[kind])])
        assert int((~keep).sum()) == int(res["removed"][kind])
        assert same_rows(cs.sorted_rows(after[kind]), cs.sorted_rows(before[kind][keep])), "the map is the map before minus the removed set"
    # table and occupancy blocks keep no trace: no tombstones, as many keys as map points, and a query around a removed point does not return it
    mh = h.map_health()
    assert mh["purged"] == (0, 0) and mh["keys"] == (after[0].shape[0], after[1].shape[0]) and mh["block_keys"][0] <= mh0["block_keys"][0]
    assert h.health()["rebuilds"] == hl0["rebuilds"] + sum(1 for kind in (0, 1) if res["removed"][kind] > 0)
    xyzi, d2, cnt = h.map_query(removed[:64], k=8, max_radius=0.45, kind=2)
    for i in range(xyzi.shape[0]):
        for j in range(int(cnt[i])):
            assert xyzi[i, j].tobytes() not in gone
    assert (h.map_query(reference["removed"][:64], k=1, max_radius=1e-3, kind=2)[2] == 0).all()
    # a second carve with the same inputs removes nothing
    removed2, res2 = h.map_carve(cs_, poses, apply=True, **cs.CARVE)
    assert removed2.shape[0] == 0 and res2["removed"].tolist() == [0, 0] and res2["n_removed_out"] == 0
    assert res2["examined"].tolist() == [after[0].shape[0], after[1].shape[0]]
    # checkpoint save -> load into a fresh handle gives the same map
    h2 = handle(vl, **(dict(map_grow=1, map_capacity_log2=14) if grow else {}))
    h2.restore(h.checkpoint())
    for kind in (0, 1):
        assert same_rows(h2.get_map_kind(kind), after[kind])
    # two further sweeps: VLOAM_OK (sync raises otherwise), finite poses, nothing degraded; the restored handle walks the same way
    for hh in (h, h2):
        drive(hh, scene, cs.N_BUILD, cs.N_ALL)
    tj, tj2 = h.trajectory(), h2.trajectory()
    assert tj.shape[0] == cs.N_ALL and np.isfinite(tj).all() and np.array_equal(tj[cs.N_BUILD:], tj2[-2:])
    hl = h.health()
    assert hl["fallback_solves"] == hl0["fallback_solves"] and hl["one_workgroup_solves"] == hl0["one_workgroup_solves"]
    assert h.map_health()["purged"] == (0, 0)
    final = [h.get_map_kind(kind) for kind in (0, 1)]
    for kind in (0, 1):
        assert same_rows(final[kind], h2.get_map_kind(kind)) and final[kind].shape[0] > after[kind].shape[0]
    h.close()
    h2.close()


def test_limits_and_refusals(vl, scene, reference):
    L = vl.lib()
    hb = vl.Handle(0, n_sessions=2, scan_line=cs.RINGS, with_mapping=1, max_points=cs.MAX_POINTS, max_frames=16, **cs.PARAMS)
    for k in range(cs.N_BUILD):
        hb.batch_process_scan([scene[k], scene[k]])
    hb.sync()
    cs_, poses = [scene[k] for k in cs.CARVE_SWEEPS], reference["poses"]
    with pytest.raises(vl.VloamError) as e:
        hb.map_carve(cs_, poses, apply=True, cap=4096, **cs.CARVE)
    assert e.value.status == vl.ERR_INVALID and "the handle has 2 sessions" in str(e.value)
    removed, res = hb.select(1).map_carve(cs_, poses, **cs.CARVE)   # a dry run works on the selected session
    assert same_rows(cs.sorted_rows(removed), cs.sorted_rows(reference["removed"]))
    hb.close()

    h = handle(vl)
    drive(h, scene, 0, cs.N_BUILD)
    before = [h.get_map_kind(kind) for kind in (0, 1)]
    with pytest.raises(vl.VloamError) as e:
        h.map_carve([scene[3]] * 17, np.tile(poses[:1], (17, 1)), **cs.CARVE)
    assert e.value.status == vl.ERR_INVALID and "n_sweeps must be 1 .. 16" in str(e.value)
    bad = poses.copy()
    bad[1, 5] = np.nan
    with pytest.raises(vl.VloamError) as e:
        h.map_carve(cs_, bad, apply=True, **cs.CARVE)
    assert e.value.status == vl.ERR_INVALID and "pose 1, component 5 is not finite" in str(e.value)
    # a list that is too small: VLOAM_ERR_CAPACITY, the need reported, nothing applied
    n_need = reference["removed"].shape[0]
    opt = h._carve_options(True, **cs.CARVE)
    clouds = [np.ascontiguousarray(c) for c in cs_]
    ptrs = (C.c_void_p * 2)(*[c.ctypes.data for c in clouds])
    n = (C.c_int * 2)(*[c.shape[0] for c in clouds])
    buf = np.zeros((n_need - 1, 4), np.float32)
    out = np.zeros(1, vl.CARVE_RESULT_DTYPE)
    st = L.vloam_map_carve(h.h, C.byref(opt), ptrs, n, poses.ctypes.data_as(C.c_void_p), 2, buf.ctypes.data_as(C.c_void_p), C.c_longlong(n_need - 1),
                           out.ctypes.data_as(C.c_void_p))
    assert st == vl.ERR_CAPACITY and int(out[0]["n_removed_out"]) == n_need and b"nothing was applied" in L.vloam_last_error()
    assert out[0]["removed"].tolist() == reference["res"]["removed"].tolist()
    for kind in (0, 1):
        assert same_rows(h.get_map_kind(kind), before[kind])
    assert h.map_health()["purged"] == (0, 0)
    # the smallest image; a sweep without a valid point; the last mapped pose in place of a pose
    small = dict(cs.CARVE, rows=1, cols=4)
    removed, res = h.map_carve(cs_, poses, **small)
    model = [cm.carve(before[kind], cs_, poses, **small) for kind in (0, 1)]
    assert [int(v) for v in res["removed"]] == [m[1]["removed"] for m in model] and [int(v) for v in res["in_view"]] == [m[1]["in_view"] for m in model]
    assert same_rows(cs.sorted_rows(removed), cs.sorted_rows(np.concatenate([before[kind][model[kind][0]] for kind in (0, 1)])))
    blind = np.full((64, 4), np.nan, np.float32)
    for sw in (blind, np.zeros((0, 4), np.float32)):
        removed, res = h.map_carve([sw], poses[1:], apply=True, **cs.CARVE)
        assert removed.shape[0] == 0 and res["removed"].tolist() == [0, 0] and res["seen_through"].tolist() == [0, 0]
        assert res["examined"].tolist() == [before[0].shape[0], before[1].shape[0]]
    last_pose, last_given = h.map_carve([scene[4]], None, **cs.CARVE), h.map_carve([scene[4]], poses[1:], **cs.CARVE)
    assert same_rows(cs.sorted_rows(last_pose[0]), cs.sorted_rows(last_given[0])) and last_pose[0].shape[0] > 0
    # the device form: the same set from device tensors into a device list
    import torch
    dev = [torch.from_numpy(c).cuda() for c in clouds]
    d_out = torch.zeros((n_need + 8, 4), dtype=torch.float32, device="cuda")
    res = h.map_carve_device(dev, poses, d_out, **cs.CARVE)
    assert res["n_removed_out"] == n_need and same_rows(cs.sorted_rows(d_out.cpu().numpy()[:n_need]), cs.sorted_rows(reference["removed"]))
    for kind in (0, 1):
        assert same_rows(h.get_map_kind(kind), before[kind])
    h.close()


def test_a_handle_that_never_carves_is_untouched(vl, scene):
    def run(carve_after=None):
        h = handle(vl, sweep_log=1)
        for k in range(cs.N_ALL):
            h.process_scan(scene[k])
            if k + 1 == carve_after:   # a dry run in mid-sequence
                h.sync()
                assert h.map_carve(*carve_args(h, scene), **cs.CARVE)[0].shape[0] > 0
        h.sync()
        out = h.trajectory().tobytes(), h.get_map().tobytes(), h.sweep_log().tobytes()
        h.close()
        return out

    base = run()
    other = handle(vl)   # another handle of the process carves for good meanwhile
    drive(other, scene, 0, cs.N_BUILD)
    assert other.map_carve(*carve_args(other, scene), apply=True, **cs.CARVE)[0].shape[0] > 0
    assert run() == base, "a handle that never carves"
    other.close()
    assert run(carve_after=cs.N_BUILD) == base, "a dry run writes nothing the sequence owns"
