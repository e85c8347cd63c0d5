"""-m gpu: localisation (vloam_map_localize / vloam_map_localize_device) — a dry run of the mapping stage against the map as it is.

What is checked: the dry run of the sweep in progress is bit for bit the mapping that follows; no call changes anything the sequence can see;
foreign clouds under a foreign pose agree with the CPU oracle's LaserMapping::input + solveMapping at the tolerance
tests/test_gpu_stage_inputs.py applies to vloam_set_mapping_input poses; a pose that would roll the cube window is reported and rolls nothing;
a thin map gates the solve; a restored map answers like the one that was saved; the device form equals the host form."""
import numpy as np
import pytest

import branch_cases
from test_gpu_laser_mapping import qdist
from test_gpu_stage_inputs import POSE_TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings a HIP runtime of its own: up before this module's first handle (tests/test_gpu_host_input.py); the device form takes tensors."""
    import torch
    torch.zeros(1).cuda()


def bits(v):
    return np.ascontiguousarray(v).tobytes()


def same_record(a, b):
    return sorted(a) == sorted(b) and all(bits(a[k]) == bits(b[k]) for k in a)


def staged_sweep(h, cloud):
    """scan registration + odometry of one sweep; the caller runs laser_mapping()"""
    h.reset_frame()
    h.scan_registration(cloud)
    return h.laser_odometry()


def rot_z(q, deg):
    a = np.deg2rad(deg) / 2.0
    r = np.array([0.0, 0.0, np.sin(a), np.cos(a)])
    x1, y1, z1, w1 = r
    x2, y2, z2, w2 = q
    out = np.array([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2,
                    w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2])
    return out / np.linalg.norm(out)


def qmul(a, b):
    x1, y1, z1, w1 = a
    x2, y2, z2, w2 = b
    return np.array([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2,
                     w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2])


def qrot(q, v):
    u, w = q[:3], q[3]
    c = 2.0 * np.cross(u, v)
    return v + w * c + np.cross(u, c)


def dry_run_is_the_mapping(vl, h, r, qm, tm, k):
    """r: the dry run of the sweep in progress; (qm, tm): what laser_mapping() of that sweep returned right behind it.  Returns whether it solved.
    (Also the assertion of tests/test_gpu_carve_raw.py, on a map that holds raw voxels.)"""
    assert bits(r["q_map"]) == bits(qm) and bits(r["t_map"]) == bits(tm), "sweep %d: dry run %s %s, mapping %s %s" % (k, r["q_map"], r["t_map"], qm, tm)
    st = h.map_state()
    assert list(r["n_stack"]) == [st["n_corner_stack"], st["n_surf_stack"]] and list(r["n_map"]) == [st["n_map_corner"], st["n_map_surf"]]
    assert list(r["center_cube"]) == list(st["centerCube"])
    assert bool(r["flags"] & vl.LOC_SOLVED) == bool(st["do_optimize"]) and bool(r["flags"] & vl.LOC_NOT_OPTIMIZED) != bool(st["do_optimize"])
    assert r["error_bits"] == 0 and not r["flags"] & (vl.LOC_WOULD_ROLL | vl.LOC_DEGRADED)
    if st["do_optimize"]:
        for outer in (0, 1):
            d = h.map_debug(outer)
            assert list(r["n_factors"][outer]) == [d["corner_idx"].size, d["surf_idx"].size], (k, outer)
            assert r["iterations"][outer] == d["rec"]["trace"].shape[0] and r["termination"][outer] == d["rec"]["termination"]
            assert bits(r["initial_cost"][outer]) == bits(np.float64(d["rec"]["initial_cost"])) and bits(r["final_cost"][outer]) == bits(np.float64(d["rec"]["final_cost"]))
        assert bits(r["q_guess"]) != bits(r["q_map"]) or bits(r["t_guess"]) != bits(r["t_map"])
    return bool(st["do_optimize"])


def test_dry_run_of_the_sweep_in_progress_is_the_mapping_that_follows(vl, sweeps):
    h = vl.Handle(0, with_mapping=1)
    solved = 0
    for k in range(5):
        staged_sweep(h, sweeps(64, 256, k))
        r = h.map_localize(None, None, None, None) if k >= 1 else None
        qm, tm = h.laser_mapping()
        if r is None:
            continue
        solved += dry_run_is_the_mapping(vl, h, r, qm, tm, k)
    assert solved >= 3, solved
    h.close()


def test_nothing_of_the_sequence_moves(vl, sweeps):
    def drive(localize):
        h = vl.Handle(0, scan_line=16, with_mapping=1, sweep_log=1)
        seen = []
        last = (np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3))
        for k in range(6):
            qw, tw, _, _ = staged_sweep(h, sweeps(16, 256, k))
            if localize:
                corner, surf = h.features(5), h.features(6)
                seen.append(h.map_localize(None, None, None, None))
                seen.append(h.map_localize(corner[::2], surf[1::2], rot_z(last[0], 2.0), last[1] + np.array([0.3, 0.0, 0.0]), pose_frame=1))
                seen.append(h.map_localize(corner, surf, last[0], last[1] + np.array([400.0, 0.0, 0.0]), pose_frame=1))
                seen.append(h.map_localize(corner, surf[::3], qw, tw))
            last = h.laser_mapping()
        h.sync()   # raises on a sticky error word
        out = dict(traj=h.trajectory(), map=h.get_map(), counts=h.counts(), health=h.health(), log=h.sweep_log(), state=h.map_state())
        h.close()
        return out, seen
    a, seen = drive(True)
    b, _ = drive(False)
    assert bits(a["traj"]) == bits(b["traj"]) and a["traj"].shape == (6, 14)
    assert a["map"].shape == b["map"].shape and bits(a["map"]) == bits(b["map"]) and a["map"].shape[0] > 500
    assert a["counts"] == b["counts"] and a["health"] == b["health"]
    assert bits(a["log"]) == bits(b["log"]) and not a["log"]["error_bits"].any()
    assert all(bits(a["state"][k]) == bits(b["state"][k]) for k in a["state"])
    # ... and the calls did something: far-away guesses see no map and would roll, near ones solve once the map is dense enough
    far = seen[2::4]
    assert all(r["flags"] & vl.LOC_NOT_OPTIMIZED and r["flags"] & vl.LOC_WOULD_ROLL and bits(r["q_map"]) == bits(r["q_guess"]) for r in far)
    assert sum(1 for r in seen[1::4] if r["flags"] & vl.LOC_SOLVED) >= 3 and sum(1 for r in seen[3::4] if r["flags"] & vl.LOC_SOLVED) >= 3
    assert all(r["error_bits"] == 0 for r in seen)


def test_foreign_clouds_against_the_oracle(vl, orc, sweeps):
    k = 3
    h = vl.Handle(0, with_mapping=1)
    o = orc.Oracle(with_mapping=True)
    src = vl.Handle(0, with_mapping=1)   # the second handle: sweep k's clouds and odometry pose
    for i in range(k):
        c = sweeps(64, 256, i)
        staged_sweep(h, c)
        h.laser_mapping()
        staged_sweep(src, c)
        src.laser_mapping()
        assert o.stage_sr(c) == 0
        o.stage_lo()
        assert o.stage_map() == 0
    c = sweeps(64, 256, k)
    qw, tw, _, _ = staged_sweep(src, c)
    corner, surf, full = src.features(5), src.features(6), src.features(0)
    q2 = qw + np.array([1e-3, -2e-3, 5e-4, 0.0])
    q2 = q2 / np.linalg.norm(q2)
    t2 = tw + np.array([0.02, -0.01, 0.005])
    assert o.stage_sr(c) == 0
    o.stage_lo()
    assert o.stage_map(corner=corner, surf=surf, full=full, q=q2, t=t2) == 0
    oq, ot, _, _ = o.map_pose()
    before = h.map_state()
    r = h.map_localize(corner, surf, q2, t2)
    assert r["flags"] & vl.LOC_SOLVED and r["error_bits"] == 0
    print("localise vs oracle: |dq| %.3e |dt| %.3e" % (qdist(r["q_map"], oq), np.linalg.norm(r["t_map"] - ot)))
    assert qdist(r["q_map"], oq) < POSE_TOL and np.linalg.norm(r["t_map"] - ot) < POSE_TOL
    for outer in (0, 1):
        s = o.map_solve(outer)
        assert list(r["n_factors"][outer]) == [s["corner_num"], s["surf_num"]], outer
        assert r["termination"][outer] == s["termination"] and r["iterations"][outer] == s["trace"].shape[0]
    # pose_frame 1: the same guess, formed on the host in f64
    g_q = qmul(before["q_wmap_wodom"], q2)
    g_t = qrot(before["q_wmap_wodom"], t2) + before["t_wmap_wodom"]
    g_q = g_q / np.linalg.norm(g_q)
    r1 = h.map_localize(corner, surf, g_q, g_t, pose_frame=1)
    assert r1["flags"] & vl.LOC_SOLVED
    assert qdist(r1["q_map"], oq) < POSE_TOL and np.linalg.norm(r1["t_map"] - ot) < POSE_TOL
    assert qdist(r1["q_guess"], r["q_guess"]) < 1e-12 and np.linalg.norm(r1["t_guess"] - r["t_guess"]) < 1e-12
    after = h.map_state()
    assert all(bits(before[key]) == bits(after[key]) for key in before)
    h.close()
    src.close()


def test_a_pose_that_would_roll_the_window(vl, synth):
    walk = branch_cases.six_way_walk()
    seq = synth.SynthSequence(n_rings=64, n_azimuth=256, n_sweeps=len(walk))
    h = vl.Handle(0, with_mapping=1)
    rolled_at = None
    for k in range(len(walk)):
        qw, tw, _, _ = staged_sweep(h, seq.sweep(k))
        h.set_mapping_input(q_wodom_curr=qw, t_wodom_curr=tw + walk[k])
        cen0 = h.map_state()["cen"]
        r = h.map_localize(None, None, None, None)
        cen1 = h.map_state()["cen"]
        assert np.array_equal(cen0, cen1), "the dry run moved the window, sweep %d" % k
        qm, tm = h.laser_mapping()
        st = h.map_state()
        assert bits(r["q_map"]) == bits(qm) and bits(r["t_map"]) == bits(tm), "sweep %d" % k
        assert list(r["center_cube"]) == list(st["centerCube"]) and list(r["n_map"]) == [st["n_map_corner"], st["n_map_surf"]]
        assert bool(r["flags"] & vl.LOC_WOULD_ROLL) == (not np.array_equal(st["cen"], cen0)), "sweep %d" % k
        if r["flags"] & vl.LOC_WOULD_ROLL:
            rolled_at = k
            break
    assert rolled_at is not None and rolled_at >= 3, rolled_at
    h.close()


def test_thin_map_gates_the_solve(vl, sweeps):
    src = vl.Handle(0, with_mapping=0)   # the recipe for raw sweeps: scan registration on a handle without mapping
    src.scan_registration(sweeps(64, 256, 0))
    corner, surf = src.features(2), src.features(4)
    src.close()
    assert corner.shape[0] > 50 and surf.shape[0] > 500
    h = vl.Handle(0, with_mapping=1)
    q = rot_z(np.array([0.0, 0.0, 0.0, 1.0]), 5.0)
    r = h.map_localize(corner, surf, q, np.array([1.0, 2.0, 0.5]))
    assert r["flags"] == vl.LOC_NOT_OPTIMIZED and r["error_bits"] == 0 and list(r["n_map"]) == [0, 0]
    assert bits(r["q_map"]) == bits(r["q_guess"]) and bits(r["t_map"]) == bits(r["t_guess"]) and bits(r["q_guess"]) == bits(q)
    assert r["n_stack"][0] > 10 and r["n_stack"][1] > 50
    with pytest.raises(vl.VloamError) as e:   # no sweep in progress
        h.map_localize(None, None, None, None)
    assert e.value.status == vl.ERR_ORDER
    staged_sweep(h, sweeps(64, 256, 0))
    r = h.map_localize(None, None, None, None)
    assert r["flags"] == vl.LOC_NOT_OPTIMIZED and r["error_bits"] == 0
    assert bits(r["q_map"]) == bits(r["q_guess"]) and bits(r["t_map"]) == bits(r["t_guess"])
    qm, tm = h.laser_mapping()
    assert bits(r["q_map"]) == bits(qm) and bits(r["t_map"]) == bits(tm)
    h.sync()
    h.close()


def test_restored_maps_answer_alike(vl, sweeps):
    h = vl.Handle(0, with_mapping=1, map_capacity_log2=20)
    for k in range(4):
        staged_sweep(h, sweeps(64, 256, k))
        q, t = h.laser_mapping()
    corner, surf = h.features(5)[::2], h.features(6)[::2]
    ckpt = h.checkpoint()
    guess = (rot_z(q, 1.0), t + np.array([0.2, -0.1, 0.05]))
    want = h.map_localize(corner, surf, guess[0], guess[1], pose_frame=1)
    want0 = h.map_localize(corner, surf, guess[0], guess[1], pose_frame=0)
    assert want["flags"] & vl.LOC_SOLVED and want0["flags"] & vl.LOC_SOLVED
    h.close()
    for kw in (dict(map_capacity_log2=18), dict(map_capacity_log2=14, map_grow=1)):
        h2 = vl.Handle(0, with_mapping=1, **kw)
        h2.restore(ckpt)
        got = h2.map_localize(corner, surf, guess[0], guess[1], pose_frame=1)
        got0 = h2.map_localize(corner, surf, guess[0], guess[1], pose_frame=0)
        assert same_record(got, want) and same_record(got0, want0), (kw, got, want)
        h2.close()


def test_device_form(vl, sweeps):
    import torch
    clouds = [torch.from_numpy(np.ascontiguousarray(sweeps(64, 256, k))).cuda() for k in range(5)]

    def drive(localize):
        h = vl.Handle(0, with_mapping=1)
        rec = None
        for k in range(5):
            if localize and k == 3:
                h.sync()
                tj = h.trajectory()
                corner, surf = h.features(5)[::2].copy(), h.features(6)[1::2].copy()
                q, t = tj[2, 7:11].copy(), tj[2, 11:14] + np.array([0.1, 0.1, 0.0])
                host = h.map_localize(corner, surf, q, t, pose_frame=1)
                d_corner, d_surf = torch.from_numpy(corner).cuda(), torch.from_numpy(surf).cuda()
                d_res = torch.zeros(vl.LOCALIZE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                h.map_localize_device(d_corner, d_surf, q, t, d_res, pose_frame=1)
                rec = (host, d_res, d_corner, d_surf)
            h.process_scan_device(clouds[k].data_ptr(), clouds[k].shape[0])   # right behind the call
        h.sync()
        tj = h.trajectory()
        h.close()
        return tj, rec
    tj_a, (host, d_res, _, _) = drive(True)
    tj_b, _ = drive(False)
    dev = d_res.cpu().numpy().view(vl.LOCALIZE_RESULT_DTYPE)[0]
    assert host["flags"] & vl.LOC_SOLVED
    for key in host:
        assert bits(np.asarray(host[key], dev[key].dtype)) == bits(dev[key]), key
    assert tj_a.shape == (5, 14) and bits(tj_a) == bits(tj_b)
