"""The preconditions of the raw-voxel GPU tests (tests/test_gpu_archive_tails.py, tests/test_gpu_carve_raw.py), from the CPU oracle alone:
the 140 m six-way walk of tests/raw_tail_cases.py evicts un-merged arrivals of both kinds, in groups that are all tail and in groups where a
filtered prefix comes first, and the first leg leaves raw voxels inside the window.  No GPU test can pass on nothing."""
import numpy as np
import pytest

import map_archive_cases as cases
import raw_tail_cases as rt

# un-merged rows evicted, per kind and sweep
TAIL_ROWS = {0: {40: 2, 41: 1, 48: 9, 49: 1, 51: 9, 52: 6, 54: 3, 57: 60, 58: 28}, 1: {57: 3, 58: 3}}
# all rows evicted, per kind and sweep
ROWS = {0: {40: 25, 41: 318, 42: 3716, 48: 67, 49: 6794, 51: 3663, 52: 7125, 54: 13031, 57: 14224, 58: 5948},
        1: {41: 63, 42: 1918, 48: 4, 49: 3747, 51: 2016, 52: 3875, 54: 7027, 57: 7253, 58: 3773}}
# raw voxels inside the window behind each sweep, [corner, surf]
RAW_VOXELS = [[13, 0], [20, 0], [23, 0], [21, 0], [25, 1], [34, 7], [43, 14], [55, 16], [53, 22], [58, 34], [59, 26], [68, 26], [93, 27], [91, 32],
              [110, 49], [116, 49], [120, 49], [130, 49], [119, 49], [127, 50], [133, 50], [160, 52], [177, 52], [187, 52], [195, 52], [195, 52],
              [196, 52], [195, 52], [188, 52], [175, 52], [168, 50], [162, 49], [170, 49], [175, 49], [184, 51], [171, 43], [177, 48], [194, 57],
              [203, 62], [212, 62], [217, 64], [239, 68], [258, 68], [283, 68], [312, 70], [337, 70], [365, 70], [387, 71], [407, 71], [410, 71],
              [413, 71], [419, 85], [440, 71], [448, 78], [469, 71], [491, 71], [532, 78], [488, 68], [550, 68]]


@pytest.fixture(scope="module")
def ref(orc, synth):
    before = synth.MAX_RANGE
    r = rt.walk_reference(orc, synth)
    assert synth.MAX_RANGE == before, "the sensor model's range is restored"
    return r


def test_the_walk_evicts_un_merged_arrivals(ref):
    f = rt.figures(ref)
    print(f)
    assert f["tail_rows"] >= 100
    assert f["mixed"] >= 5, "groups with a filtered prefix and a tail"
    assert f["all_tail"] >= 1
    assert min(f["tail_rows_of_kind"]) >= 1
    assert f["tail_rows_per_sweep"] == TAIL_ROWS
    assert f["rows_per_sweep"] == ROWS
    assert f["raw_voxels_per_sweep"] == RAW_VOXELS
    assert (f["groups"], f["rows"], f["tail_rows"], f["groups_with_tail"], f["mixed"], f["all_tail"], f["first_evicting"]) == (385, 84587, 125, 25, 7, 18, 40)
    assert sum(RAW_VOXELS[rt.N_CARVE - 1]) > 0, "the first leg leaves raw voxels in the window"


def test_the_bookkeeping_is_consistent(ref):
    for sweep, kind, cube, pts, tail in rt.groups(ref):
        assert 0 <= tail <= pts.shape[0] and pts.shape[0] > 0
        if tail:
            # what one sweep brought into one voxel of a cube outside the valid block stays apart; a filtered prefix holds one point per voxel
            head = rt.voxel_rows(pts[:pts.shape[0] - tail], kind)
            assert np.unique(head, axis=0).shape[0] == head.shape[0], (sweep, kind, cube)
    for k, per_kind in enumerate(ref["raw"]):
        for kind in (0, 1):
            w = per_kind[kind]["cube"] + ref["cen"][k]
            assert ((w >= 0) & (w < cases.SIZE)).all(), "tail points lie inside the window"
            assert rt.raw_voxels(ref, k, kind).shape[0] <= per_kind[kind]["points"].shape[0]


def test_out_and_back(orc, synth):
    """the drive of tests/test_gpu_carve_raw.py: raw voxels of both kinds behind sweep 6, new ones on sweeps 6 and 7, fewer once the way back
    brings their cubes into the valid block again; nothing leaves the window"""
    r = rt.out_and_back_reference(orc, synth)
    counts = rt.figures(r)["raw_voxels_per_sweep"]
    assert counts == [[11, 1], [17, 1], [24, 1], [29, 1], [29, 1], [36, 6], [48, 15], [57, 17], [71, 17], [82, 19], [51, 16], [55, 16], [56, 16]]
    assert not r["expected"] and len(r["walk"]) == rt.N_CARVE + rt.N_BACK
    k = rt.N_CARVE - 1
    assert all(counts[k - 1][kind] < counts[k][kind] < counts[k + 1][kind] for kind in (0, 1))
    assert any(counts[i + 1][kind] < counts[i][kind] for i in range(k, len(counts) - 1) for kind in (0, 1))
    assert all(m.shape[0] > 10000 for m in r["map_after"][k])


def test_the_plain_walk_is_what_it_was(orc, synth):
    """the parameters default to the walk tests/test_gpu_map_archive.py pins (its EXPECTED), and both walks live side by side in one process"""
    r = cases.walk_reference(orc, synth)
    assert cases.expected_counts(r) == {0: {41: 88, 42: 2492, 55: 1525, 56: 25250, 57: 68327, 58: 26497}, 1: {41: 2, 42: 1257, 55: 514, 56: 14685, 57: 34983, 58: 14407}}
    assert "raw" not in r and len(r["expected"]) == 346
