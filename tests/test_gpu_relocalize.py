"""-m gpu: coarse-to-fine relocalisation (vloam_map_relocalize) — the grid, the ranking and the records against the numpy model of
tests/pose_score_model.py, the refinements against vloam_map_localize called separately, and the refusals of both new calls against a handle."""
import numpy as np
import pytest

import pose_score_model as model
from test_gpu_pose_score import bits, features_of, leaf_bounds, scene, thin, torch_first   # noqa: F401 (fixtures: the five-sweep scene)

pytestmark = pytest.mark.gpu
F32 = np.float32
GRID = dict(n_xy=(9, 9), n_z=1, n_yaw=9, half_extent=(2.0, 2.0, 0.0), half_yaw=float(np.deg2rad(10.0)))   # 0.5 m and 2.5 degree steps
HALF_STEP_T, HALF_STEP_YAW = 0.25, float(np.deg2rad(1.25))


def yaw_between(qa, qb):
    """Rotation angle of qb * qa^-1."""
    d = abs(float(np.dot(qa, qb))) / (np.linalg.norm(qa) * np.linalg.norm(qb))
    return 2.0 * np.arccos(min(1.0, d))


def offset_centre(true, dt, ddeg):
    q = model.qmul(model.yaw_quat(np.deg2rad(ddeg)), true[:4])
    return q / np.linalg.norm(q), true[4:] + np.asarray(dt, np.float64)


# ------------------------------------------------------------------------------------------------ 6. consistency
def test_records_ranking_and_refinements(vl, scene):
    d, h = scene, scene["h"]
    rng = np.random.default_rng(31)
    true = d["poses"][0]
    qc, tc = offset_centre(true, (0.7, -0.4, 0.0), 3.0)
    r = h.map_relocalize(d["corner"], d["surf"], qc, tc, top_k=4, **GRID)
    assert r["n_candidates"] == 729 and r["n_refined"] == 4 and 0 <= r["best"] < 4 and len(set(r["candidate"].tolist())) == 4
    others = [int(m) for m in rng.choice(729, 40, replace=False) if m not in r["candidate"].tolist()][:32]
    idx = r["candidate"].tolist() + others
    poses = np.array([np.concatenate(model.grid_pose(m, qc, tc, **GRID)) for m in idx])
    want = model.score_poses(d["maps"], d["corner"], d["surf"], poses)
    for j in range(4):
        assert bits(r["coarse"][j]) == bits(want[j]), "coarse[%d] (candidate %d): device %s model %s" % (j, idx[j], r["coarse"][j], want[j])
        if j:
            assert model.before(want[j - 1], idx[j - 1], want[j], idx[j]), "candidate[] is in ranking order"
    got_others = h.map_score_poses(d["corner"], d["surf"], poses[4:])
    assert bits(got_others) == bits(want[4:]), "the records of 32 other candidates"
    for j in range(4, len(idx)):
        assert model.before(want[3], idx[3], want[j], idx[j]), "candidate %d outranks candidate[3]" % idx[j]
    for j in range(4):
        q, t = model.grid_pose(idx[j], qc, tc, **GRID)
        ref = r["refined"][j]
        assert np.abs(ref["q_guess"] - q).max() <= 1e-12 and np.abs(ref["t_guess"] - t).max() <= 1e-12, "candidate %d: the guess" % idx[j]
        sep = h.map_localize(d["corner"], d["surf"], ref["q_guess"], ref["t_guess"], pose_frame=1)
        assert sorted(sep) == sorted(ref) and all(bits(sep[k]) == bits(ref[k]) for k in sep), "refined[%d] is map_localize from that guess" % j
    fine_poses = np.array([np.concatenate([ref["q_map"], ref["t_map"]]) for ref in r["refined"]])
    fine = model.score_poses(d["maps"], d["corner"], d["surf"], fine_poses)
    assert bits(r["fine"]) == bits(fine), (r["fine"], fine)
    assert r["best"] == int(model.rank(fine)[0])
    h.sync()


# ------------------------------------------------------------------------------------------------ 7. it does what it is for
def test_finds_the_pose_from_a_centre_plain_localisation_fails_from(vl, orc, scene):
    """The centre is the sweep's true map pose moved by (1.5, -1.0, 0) m and 8 degrees of yaw; the bound is half a coarse step (0.25 m, 1.25
    degrees) around what map_localize returns from the true pose.
    First, on the CPU and without the library: the CPU oracle maps the same five sweeps, and the numpy model scores all 729 candidates of the
    grid against the ORACLE's map around the ORACLE's pose of the fifth sweep, on every eighth corner and every sixteenth surf point of the
    thinned clouds (24 + 48 points: enough to rank a grid whose neighbours differ by 0.5 m, and what keeps the brute force at seconds).  Its
    winner must be the grid point nearest the truth or a direct neighbour; it is, for this scene and sweep (SynthSequence(64, 256), sweep 4),
    so no other sweep or seed was needed.
    Measured on an MI355X with this scene: plain map_localize from the offset centre reports VLOAM_LOC_SOLVED and ends 1.837 m and 7.45
    degrees from the goal, the wrong basin; the coarse winner is the grid point nearest the truth (136), and refined[best] ends 0.098 m and
    0.014 degrees from the goal."""
    d, h = scene, scene["h"]
    # the grid point nearest the truth: offsets (-1.5, +1.0) m and -8 degrees from the centre -> steps (1, 6) of 0 .. 8 in x, y; yaw -7.5 degrees: step 1
    near = 1 + 9 * (6 + 9 * 1)
    cand = [near + dx + 9 * dy + 81 * dyaw for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dyaw in (-1, 0, 1)]
    o = orc.Oracle(with_mapping=True)
    for k in range(5):
        assert o.process(d["clouds"][k]) == 0
    oq, ot, _, _ = o.map_pose()
    omaps = tuple(np.concatenate([o.map_cube(kind, c) for c in range(21 * 21 * 11)]).astype(F32) for kind in (0, 1))
    assert omaps[0].shape[0] > 500 and omaps[1].shape[0] > 500
    oqc, otc = offset_centre(np.concatenate([oq / np.linalg.norm(oq), ot]), (1.5, -1.0, 0.0), 8.0)
    grid = np.array([np.concatenate(model.grid_pose(m, oqc, otc, **GRID)) for m in range(729)])
    winner = int(model.rank(model.score_poses(omaps, d["corner"][::8], d["surf"][::16], grid))[0])
    print("the model's coarse winner on the oracle's map: %d (nearest grid point %d)" % (winner, near))
    assert winner in cand, "the scene does not single out the truth: the model's winner on the oracle's map is %d" % winner
    # ... then the device
    true = d["poses"][0]
    goal = h.map_localize(d["corner"], d["surf"], true[:4], true[4:], pose_frame=1)
    assert goal["flags"] & vl.LOC_SOLVED
    qc, tc = offset_centre(true, (1.5, -1.0, 0.0), 8.0)
    plain = h.map_localize(d["corner"], d["surf"], qc, tc, pose_frame=1)
    miss_t, miss_yaw = np.linalg.norm(plain["t_map"] - goal["t_map"]), yaw_between(plain["q_map"], goal["q_map"])
    print("plain map_localize from the offset centre: flags %d, %.3f m and %.2f degrees from the goal" % (plain["flags"], miss_t, np.rad2deg(miss_yaw)))
    r = h.map_relocalize(d["corner"], d["surf"], qc, tc, top_k=4, **GRID)
    print("relocalise: candidates %s (nearest grid point %d), coarse hits %s, fine hits %s, best %d" %
          (r["candidate"].tolist(), near, r["coarse"]["n_hit"].tolist(), r["fine"]["n_hit"].tolist(), r["best"]))
    assert r["candidate"][0] in cand, "the coarse winner %d is no neighbour of the grid point nearest the truth (%d)" % (r["candidate"][0], near)
    best = r["refined"][r["best"]]
    dt, dyaw = np.linalg.norm(best["t_map"] - goal["t_map"]), yaw_between(best["q_map"], goal["q_map"])
    print("refined[best]: %.4f m and %.3f degrees from the goal" % (dt, np.rad2deg(dyaw)))
    assert dt <= HALF_STEP_T and dyaw <= HALF_STEP_YAW
    assert miss_t > HALF_STEP_T or miss_yaw > HALF_STEP_YAW, "plain localisation already lands within the bound: the offset shows nothing"


# ------------------------------------------------------------------------------------------------ 8. refusals against the handle
def test_refusals_leave_the_handle_usable(vl, scene):
    d, h = scene, scene["h"]
    ok = h.map_score_poses(d["corner"], d["surf"], d["poses"][:4])

    def refused(fn, status, *words):
        with pytest.raises(vl.VloamError) as e:
            fn()
        assert e.value.status == status and all(w in str(e.value) for w in words), str(e.value)
        assert bits(h.map_score_poses(d["corner"], d["surf"], d["poses"][:4])) == bits(ok), "the handle stays usable"

    up = lambda v: float(np.nextafter(F32(v), F32(np.inf)))
    lb = leaf_bounds(h)
    refused(lambda: h.map_score_poses(d["corner"], d["surf"], d["poses"], radius=(up(lb[0]), 1.0)), vl.ERR_INVALID, "radius[0]", "16 leaves of the corner map", "at most 6.4")
    refused(lambda: h.map_score_poses(d["corner"], d["surf"], d["poses"], radius=(1.0, up(lb[1]))), vl.ERR_INVALID, "radius[1]", "16 leaves of the surf map", "at most 12.8")
    refused(lambda: h.map_relocalize(d["corner"], d["surf"], d["poses"][0, :4], d["poses"][0, 4:], radius=(1.0, up(lb[1]))), vl.ERR_INVALID, "vloam_map_relocalize", "at most 12.8")
    refused(lambda: h.map_score_poses(d["corner"], d["surf"], d["poses"], stride=(0, 1)), vl.ERR_INVALID, "stride[0]")
    refused(lambda: h.map_score_poses(d["corner"], d["surf"], d["poses"], radius=(1.0, float("nan"))), vl.ERR_INVALID, "radius[1] must be positive and finite")
    refused(lambda: h.map_score_poses(d["corner"], d["surf"], np.zeros((65537, 7))), vl.ERR_INVALID, "M must be 0 .. 65536")
    bad = d["poses"][:4].copy()
    bad[2, 3] += 1e-3
    refused(lambda: h.map_score_poses(d["corner"], d["surf"], bad), vl.ERR_INVALID, "pose 2: the quaternion's norm")
    bad = d["surf"].copy()
    bad[7, 1] = np.nan
    refused(lambda: h.map_score_poses(d["corner"], bad, d["poses"][:4]), vl.ERR_INVALID, "surf cloud, point 7: component 1 is not finite")
    refused(lambda: h.map_relocalize(d["corner"], d["surf"], d["poses"][0, :4], d["poses"][0, 4:], top_k=9), vl.ERR_INVALID, "top_k must be 1 .. 8")
    refused(lambda: h.map_relocalize(d["corner"], d["surf"], d["poses"][0, :4], d["poses"][0, 4:], n_xy=(300, 300)), vl.ERR_INVALID, "more than 65536 candidates")
    big = np.zeros((64 * 256 + 1, 4), F32)
    refused(lambda: h.map_relocalize(d["corner"], big, d["poses"][0, :4], d["poses"][0, 4:]), vl.ERR_CAPACITY, "exceeds max_points")
    h.sync()
    # handles that cannot: no map, several sessions; the large stack tier scores but does not relocalise
    h0 = vl.Handle(0, with_mapping=0, max_points=64 * 256, max_frames=4)
    for fn in (lambda: h0.map_score_poses(d["corner"], d["surf"], d["poses"][:4]), lambda: h0.map_relocalize(d["corner"], d["surf"], d["poses"][0, :4], d["poses"][0, 4:])):
        with pytest.raises(vl.VloamError) as e:
            fn()
        assert e.value.status == vl.ERR_ORDER and "with_mapping == 0" in str(e.value)
    h0.close()
    hb = vl.Handle(0, n_sessions=2, with_mapping=1, max_points=64 * 256, max_frames=4)
    for fn in (lambda: hb.map_score_poses(d["corner"], d["surf"], d["poses"][:4]), lambda: hb.map_relocalize(d["corner"], d["surf"], d["poses"][0, :4], d["poses"][0, 4:])):
        with pytest.raises(vl.VloamError) as e:
            fn()
        assert e.value.status == vl.ERR_INVALID and "2 sessions" in str(e.value)
    hb.close()
    ht = vl.Handle(0, with_mapping=1, max_points=32768, max_frames=8, max_surf_stack_points=32768)
    for k in range(5):
        ht.process_scan(d["clouds"][k])
    assert bits(ht.map_score_poses(d["corner"], d["surf"], d["poses"])) == bits(h.map_score_poses(d["corner"], d["surf"], d["poses"])), "a large-tier handle scores"
    with pytest.raises(vl.VloamError) as e:
        ht.map_relocalize(d["corner"], d["surf"], d["poses"][0, :4], d["poses"][0, 4:])
    assert e.value.status == vl.ERR_INVALID and "large stack tier" in str(e.value)
    assert ht.map_score_poses(d["corner"], d["surf"], d["poses"][:1])["n_hit"].sum() > 0
    ht.sync()
    ht.close()
