"""The six-way walk of branch_cases.six_way_walk on the CPU oracle, with the bookkeeping of what each roll of the cube window evicts: the
expected rows of the map archive (vloam_map_archive_*; tests/test_gpu_map_archive.py).  Nothing here touches the device.

Before LaserMapping::input of sweep k the clouds of the cubes near the window's faces and the window position are taken; after it the
shift is cen_after - cen_before, the reference moves the cube at window index (i, j, k) to (i, j, k) + shift (laser_mapping.cpp:218-402), and
a cube whose shifted index leaves [0, size) on an axis was cleared by that sweep.  Its cloud, in the reference's order, is the expected row
sequence for (sweep, kind, absolute cube = window index - cen_before)."""
import numpy as np

import branch_cases

RINGS, N_AZ = 64, 256
W, H, D = 21, 21, 11
SIZE = np.array([W, H, D])
MAX_SHIFT = 3   # cubes per axis and sweep the bookkeeping covers (asserted: the walk's 55 m steps shift by two at most)

_cache = {}


def _near_faces():
    idx = np.arange(W * H * D)
    ijk = np.stack([idx % W, (idx // W) % H, idx // (W * H)], 1)
    near = ((ijk < MAX_SHIFT) | (ijk >= SIZE - MAX_SHIFT)).any(axis=1)
    return idx[near], ijk[near]


def walk_reference(orc, synth):
    """Run once per process: dict(walk, clouds, oq, ot, map_q, map_t, cen [n, 3], expected, final_map (callable result), first_evicting)
    expected: list of (sweep, kind, (ci, cj, ck), points float32 [m, 4]) sorted by (sweep, kind, ck, cj, ci), the archive's get order."""
    if "ref" in _cache:
        return _cache["ref"]
    from test_gpu_laser_mapping import oracle_published_map
    walk = branch_cases.six_way_walk()
    n = len(walk)
    seq = synth.SynthSequence(n_rings=RINGS, n_azimuth=N_AZ, n_sweeps=n)
    o = orc.Oracle(scan_line=RINGS, with_mapping=True)
    cand, cand_ijk = _near_faces()
    clouds, oqs, ots, mqs, mts, cens, expected = [], [], [], [], [], [], []
    for k in range(n):
        cloud = seq.sweep(k)
        clouds.append(cloud)
        assert o.stage_sr(cloud) == 0
        o.stage_lo()
        oq, ot, _, _ = o.lo_pose()
        before = o.map_info()["cen"].astype(np.int64)
        snap = {(kind, int(c)): o.map_cube(kind, int(c)).copy() for kind in (0, 1) for c in cand}
        assert o.stage_map(q=oq, t=ot + walk[k]) == 0
        after = o.map_info()["cen"].astype(np.int64)
        shift = after - before
        assert np.abs(shift).max() <= MAX_SHIFT, shift
        if shift.any():
            moved = cand_ijk + shift
            gone = ((moved < 0) | (moved >= SIZE)).any(axis=1)
            for kind in (0, 1):
                for c, ijk in zip(cand[gone], cand_ijk[gone]):
                    pts = snap[(kind, int(c))]
                    if pts.shape[0]:
                        expected.append((k, kind, tuple(int(v) for v in ijk - before), pts))
        mq, mt = o.map_published_pose()
        oqs.append(oq.copy()); ots.append(ot.copy()); mqs.append(mq.copy()); mts.append(mt.copy()); cens.append(after.copy())
    expected.sort(key=lambda e: (e[0], e[1], e[2][2], e[2][1], e[2][0]))
    ref = dict(walk=walk, clouds=clouds, oq=oqs, ot=ots, map_q=mqs, map_t=mts, cen=np.array(cens), expected=expected,
               final_map=oracle_published_map(o), first_evicting=min(e[0] for e in expected) if expected else -1)
    _cache["ref"] = ref
    return ref


def expected_counts(ref):
    """{kind: {sweep: rows}}"""
    out = {0: {}, 1: {}}
    for k, kind, _, pts in ref["expected"]:
        out[kind][k] = out[kind].get(k, 0) + pts.shape[0]
    return out
