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


def walk_reference(orc, synth, name="ref", walk=None, max_range=None, tails=False, maps_after=()):
    """Run once per process and name: dict(walk, clouds, oq, ot, map_q, map_t, cen [n, 3], expected, final_map (callable result), first_evicting)
    expected: list of (sweep, kind, (ci, cj, ck), points float32 [m, 4]) sorted by (sweep, kind, ck, cj, ci), the archive's get order.
    walk: the offsets (default: the six-way walk); max_range: the sensor model's range while the sweeps are made (default: synth's own).
    tails=True adds the bookkeeping of un-merged arrivals (tests/raw_tail_cases.py): per absolute cube and kind the number of points at the
    end of its cloud that arrived while the cube was outside the valid block and were not filtered since.  After LaserMapping::input a cube of
    map_info()["valid"] was re-filtered (tail 0); any other cube's tail grows by the growth of its cloud.  Then also
        expected_tail  [len(expected)] the tail length of each evicted group (its last rows)
        raw            per sweep {kind: dict(points float32 [m, 4]: the tail points inside the window in cube order, cube [m, 3] absolute)}
    maps_after: sweeps behind which the map is kept, per kind in get_map_kind's order: map_after[k] = [corner float32 [m, 4], surf]"""
    if name in _cache:
        return _cache[name]
    from test_gpu_laser_mapping import oracle_published_map
    import pytest
    if walk is None:
        walk = branch_cases.six_way_walk()
    n = len(walk)
    o = orc.Oracle(scan_line=RINGS, with_mapping=True)
    cand, cand_ijk = _near_faces()
    all_ijk = np.stack([np.arange(W * H * D) % W, (np.arange(W * H * D) // W) % H, np.arange(W * H * D) // (W * H)], 1)
    get_len = o.L.orc_get_map_cube
    length, tail = {}, {}      # (kind, absolute cube) -> cloud length / un-merged arrivals at its end
    clouds, oqs, ots, mqs, mts, cens, expected, raw, map_after = [], [], [], [], [], [], [], [], {}
    with pytest.MonkeyPatch.context() as mp:
        if max_range is not None:
            mp.setattr(synth, "MAX_RANGE", float(max_range))
        seq = synth.SynthSequence(n_rings=RINGS, n_azimuth=N_AZ, n_sweeps=n)
        for k in range(n):
            cloud = seq.sweep(k)
            clouds.append(cloud)
            assert o.stage_sr(cloud) == 0
            o.stage_lo()
            oq, ot, _, _ = o.lo_pose()
            before = o.map_info()["cen"].astype(np.int64)
            snap = {(kind, int(c)): o.map_cube(kind, int(c)).copy() for kind in (0, 1) for c in cand}
            assert o.stage_map(q=oq, t=ot + walk[k]) == 0
            info = o.map_info()
            after = info["cen"].astype(np.int64)
            shift = after - before
            assert np.abs(shift).max() <= MAX_SHIFT, shift
            if shift.any():
                moved = cand_ijk + shift
                gone = ((moved < 0) | (moved >= SIZE)).any(axis=1)
                for kind in (0, 1):
                    for c, ijk in zip(cand[gone], cand_ijk[gone]):
                        pts = snap[(kind, int(c))]
                        if pts.shape[0]:
                            cube = tuple(int(v) for v in ijk - before)
                            assert not tails or length[(kind, cube)] == pts.shape[0]
                            expected.append((k, kind, cube, pts, tail.get((kind, cube), 0)))
            if tails:
                valid = set(int(c) for c in info["valid"])
                new_len, new_tail, here = {}, {}, {0: ([], []), 1: ([], [])}
                for kind in (0, 1):
                    for c in range(W * H * D):
                        m = get_len(o.h, kind, c, None, 0)
                        if m == 0:
                            continue
                        cube = tuple(int(v) for v in all_ijk[c] - after)
                        new_len[(kind, cube)] = m
                        grown = m - length.get((kind, cube), 0)
                        if c not in valid:
                            assert grown >= 0, "a cube outside the valid block only takes arrivals"
                            t = tail.get((kind, cube), 0) + grown
                            if t:
                                new_tail[(kind, cube)] = t
                                here[kind][0].append(o.map_cube(kind, c)[m - t:].copy())
                                here[kind][1].append(np.repeat(np.array([cube]), t, axis=0))
                length, tail = new_len, new_tail
                raw.append({kind: dict(points=np.concatenate(here[kind][0]) if here[kind][0] else np.zeros((0, 4), np.float32),
                                       cube=np.concatenate(here[kind][1]) if here[kind][1] else np.zeros((0, 3), np.int64)) for kind in (0, 1)})
            if k in maps_after:
                map_after[k] = [np.concatenate([o.map_cube(kind, c) for c in range(W * H * D)]) for kind in (0, 1)]
            mq, mt = o.map_published_pose()
            oqs.append(oq.copy()); ots.append(ot.copy()); mqs.append(mq.copy()); mts.append(mt.copy()); cens.append(after.copy())
    expected.sort(key=lambda e: (e[0], e[1], e[2][2], e[2][1], e[2][0]))
    ref = dict(walk=walk, clouds=clouds, oq=oqs, ot=ots, map_q=mqs, map_t=mts, cen=np.array(cens), expected=[e[:4] for e in expected],
               final_map=oracle_published_map(o), first_evicting=min(e[0] for e in expected) if expected else -1)
    if tails:
        ref.update(expected_tail=[e[4] for e in expected], raw=raw)
    if maps_after:
        ref["map_after"] = map_after
    _cache[name] = ref
    return ref


def expected_counts(ref):
    """{kind: {sweep: rows}}"""
    out = {0: {}, 1: {}}
    for k, kind, _, pts in ref["expected"]:
        out[kind][k] = out[kind].get(k, 0) + pts.shape[0]
    return out
