"""-m gpu: the three movers of voxel records are interchangeable.  A tombstone rebuild of a fixed handle (k_map_rebuild_*), a growth step or
same-size rehash of a growable one (k_map_grow) and the restore of a checkpoint (k_map_ckpt_unpack) each move every live record of a table
into an empty one through one device text (csrc/map_move_dev.h), so a sequence that is moved by any of them, at any point between two sweeps,
must go on exactly as one that never was.

The drive is that of test_gpu_map_growth.test_raw_voxels_across_a_growth (64 x 512, 25 m/s, ranges up to 140 m): the suite's one drive that
leaves raw voxels, and with them entries of the deferred list, whose slot ids every move has to rewrite.  Four handles take the same sweeps:
  A  fixed, 2^17 slots, never moved
  B  fixed, 2^17, a forced rebuild after sweeps 4, 7, 10 and 13
  C  growable from 2^10, a forced growth step after sweeps 4, 7 and 13 and a forced same-size rehash after sweep 10
  D  fixed, 2^17, fresh; A's checkpoint of sweep 7 restored, then sweeps 8 .. 15
"""
import numpy as np
import pytest

from test_gpu_laser_mapping import POSE_TOL, oracle_published_map, qdist, same_cloud

pytestmark = pytest.mark.gpu

N = 16
MOVES = (4, 7, 10, 13)
SAVE_AT = 7
COUNTERS = ("keys", "purged", "deferred", "block_keys")


def counters(h, names=COUNTERS):
    mh = h.map_health()
    return {k: mh[k] for k in names}


def test_rebuild_growth_and_restore_are_interchangeable(vl, orc, synth, monkeypatch):
    monkeypatch.setattr(synth, "MAX_RANGE", 140.0)
    seq = synth.SynthSequence(n_rings=64, n_azimuth=512, n_sweeps=N + 1, speed=25.0)
    kw = dict(with_mapping=1, max_points=64 * 512)
    a = vl.Handle(0, map_capacity_log2=17, **kw)
    b = vl.Handle(0, map_capacity_log2=17, **kw)
    c = vl.Handle(0, map_capacity_log2=10, map_grow=1, **kw)
    d = vl.Handle(0, map_capacity_log2=17, **kw)
    o = orc.Oracle(with_mapping=True)
    ref, raw_at = [], {"B": [], "C": []}
    for k in range(N):
        cloud = seq.sweep(k)
        for h in (a, b, c) + ((d,) if k > SAVE_AT else ()):
            h.process_scan(cloud)
        o.process(cloud)
        qw, tw, _, _ = o.lo_pose()
        qm, tm = o.map_published_pose()
        ref.append(np.concatenate([qw, tw, qm, tm]))
        if k in MOVES:
            for name, h in (("B", b), ("C", c)):
                h.sync()
                before = counters(h)
                if name == "B" or k == 10:
                    h.map_force_rebuild()
                else:
                    lg = h.health()["map_log2"]
                    h.map_force_grow()
                    assert h.health()["map_log2"] == (lg[0] + 1, lg[1] + 1)
                h.sync()
                after = counters(h)
                print("sweep %d, %s: %s -> %s" % (k, name, before, after))
                assert after == before, "%s: the move after sweep %d changed the table's counters" % (name, k)
                raw_at[name].append(sum(before["deferred"]))
        if k == SAVE_AT:
            a.sync()
            at_save = counters(a)
            d.restore(a.checkpoint())
            d.sync()
            print("sweep %d, D: %s -> %s" % (k, at_save, counters(d)))
            assert counters(d) == at_save, "the restored tables' counters are not the saver's"
    # a move of a table without raw voxels rewrites no deferred list: at least two move points of each handle must have had some
    for name in ("B", "C"):
        assert sum(1 for r in raw_at[name] if r > 0) >= 2, (name, raw_at[name])
    for h in (a, b, c, d):
        h.sync()
    tj = {name: h.trajectory() for name, h in (("A", a), ("B", b), ("C", c), ("D", d))}
    ref = np.array(ref)
    for name, t in tj.items():
        assert t.shape == ref.shape, (name, t.shape)
        for k in range(N):
            assert qdist(t[k, 0:4], ref[k, 0:4]) < POSE_TOL and np.linalg.norm(t[k, 4:7] - ref[k, 4:7]) < POSE_TOL, "%s: LO pose, sweep %d" % (name, k)
            assert qdist(t[k, 7:11], ref[k, 7:11]) < POSE_TOL and np.linalg.norm(t[k, 11:14] - ref[k, 11:14]) < POSE_TOL, "%s: map pose, sweep %d" % (name, k)
    # ... and the same bytes: a move changes slot positions only, and nothing the sweeps compute depends on those (D over the sweeps it ran)
    for name, first in (("B", 0), ("C", 0), ("D", SAVE_AT + 1)):
        diff = [k for k in range(first, N) if tj[name][k].tobytes() != tj["A"][k].tobytes()]
        print("%s: sweeps whose pose row differs from A's in some bit: %s" % (name, diff))
        assert not diff, "%s: pose rows of sweeps %s are not A's bit for bit" % (name, diff)
    want = a.get_map()
    assert same_cloud(want, oracle_published_map(o))
    end = counters(a, ("keys", "purged", "deferred"))
    for name, h in (("B", b), ("C", c), ("D", d)):
        assert same_cloud(h.get_map(), want), "%s: the map is not A's" % name
        assert counters(h, ("keys", "purged", "deferred")) == end, (name, counters(h), end)
    for h in (a, b, c, d):
        h.close()
