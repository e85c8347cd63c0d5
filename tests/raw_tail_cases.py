"""The six-way walk of map_archive_cases with the sensor model's range raised to 140 m, on the CPU oracle: the walk whose sweeps reach cubes
outside the valid 5 x 5 x 3 block, so that the map holds UN-MERGED ARRIVALS (the reference keeps such a point unfiltered at the end of its
cube's cloud until the cube is next re-filtered; on the device: a raw voxel, csrc/map_table.h).  Nothing here touches the device.

map_archive_cases.walk_reference does the walk and the bookkeeping (tails=True); this module names the drive and reads its results:
    groups(ref)             per evicted (sweep, kind, cube): the oracle's cloud and how many of its last rows are un-merged arrivals
    raw_voxels(ref, k, kind) the raw voxels inside the window behind sweep k: the distinct voxels (voxel_key_model) of the tail points
The expected figures (tests/test_raw_tail_cases.py pins them) are the precondition of tests/test_gpu_archive_tails.py and
tests/test_gpu_carve_raw.py, which drive the device with the same clouds and the oracle's odometry poses."""
import numpy as np

import map_archive_cases as cases
import voxel_key_model

RANGE = 140.0                   # metres; synth's own 80 m reach no cube outside the valid block
LEAF = {0: 0.4, 1: 0.8}         # orc.Oracle's and vloam_create's defaults: mapping_line_resolution, mapping_plane_resolution
N_CARVE = 7                     # the first leg (55 m per sweep along -x): the drive of test_gpu_map_query.py's raw-point test


N_BACK = 6                      # ... and six sweeps that walk back through its wake: raw cubes re-enter the valid block


def walk_reference(orc, synth):
    return cases.walk_reference(orc, synth, name="raw_tails", max_range=RANGE, tails=True)


def out_and_back_reference(orc, synth):
    """The drive of tests/test_gpu_carve_raw.py: the walk's first N_CARVE offsets, then the same places in reverse (13 sweeps, no eviction).
    map_after[N_CARVE - 1] is the oracle's map where the carve, the scores and the dry runs happen."""
    walk = cases.branch_cases.six_way_walk()[:N_CARVE]
    walk = walk + walk[N_CARVE - 2::-1]
    assert len(walk) == N_CARVE + N_BACK
    return cases.walk_reference(orc, synth, name="raw_out_and_back", walk=walk, max_range=RANGE, tails=True, maps_after=(N_CARVE - 1,))


def groups(ref):
    """[(sweep, kind, cube, points, tail)] in the archive's get order"""
    return [e + (t,) for e, t in zip(ref["expected"], ref["expected_tail"])]


def voxel_rows(pts, kind):
    """int64 [n, 6]: absolute cube and voxel index (inside the whole frame, not the cube) of every point"""
    xyz = np.ascontiguousarray(np.asarray(pts)[:, :3], dtype=np.float32)
    return np.concatenate([voxel_key_model.cube_abs(xyz), voxel_key_model.voxel_index(xyz, LEAF[kind])], 1).reshape(-1, 6)


def raw_voxels(ref, sweep, kind):
    """int64 [m, 6], distinct and sorted"""
    r = ref["raw"][sweep][kind]
    rows = voxel_rows(r["points"], kind)
    assert np.array_equal(rows[:, :3], r["cube"]), "a point lies in the cube its coordinates name"
    return np.unique(rows, axis=0)


def in_voxels(pts, kind, voxels):
    """bool [n]: does the point lie in one of `voxels` (raw_voxels' rows)?"""
    have = set(map(tuple, voxels.tolist()))
    return np.array([tuple(r) in have for r in voxel_rows(pts, kind).tolist()], bool).reshape(-1)


def figures(ref):
    g = groups(ref)
    tails = [e for e in g if e[4]]
    per_sweep = {0: {}, 1: {}}
    for sweep, kind, _, _, t in tails:
        per_sweep[kind][sweep] = per_sweep[kind].get(sweep, 0) + t
    return dict(groups=len(g), rows=sum(e[3].shape[0] for e in g), tail_rows=sum(e[4] for e in g),
                tail_rows_of_kind=[sum(e[4] for e in g if e[1] == kind) for kind in (0, 1)],
                groups_with_tail=len(tails), mixed=sum(1 for e in tails if e[4] < e[3].shape[0]),
                all_tail=sum(1 for e in tails if e[4] == e[3].shape[0]), first_evicting=ref["first_evicting"],
                tail_rows_per_sweep=per_sweep, rows_per_sweep=cases.expected_counts(ref),
                raw_voxels_per_sweep=[[int(raw_voxels(ref, k, kind).shape[0]) for kind in (0, 1)] for k in range(len(ref["raw"]))])
