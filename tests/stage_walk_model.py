"""Where the odometry's adjacent-line walks break: the reference's literal walk against the device's walk-stop tables (numpy, no GPU).

The reference (laser_odometry.cpp:279-324 corner, :361-417 plane) walks the ring-sorted CornerLast / SurfLast from the closest point's index
idx upwards until the first line > r + NEARBY_SCAN and downwards until the first line < r - NEARBY_SCAN (r = int(intensity[idx]),
NEARBY_SCAN = 2.5).  The device (k_lo_grid_scan / k_lo_assoc in lo_kernels.hip) bounds every walk of line r by two stops that do not depend
on idx: stops[r + 3] = the first index of the cloud with a line >= r + 3, stops[kStopLen + r] = the last index with a line <= r - 3.
csrc/stage_input_check.h admits a substituted less-cloud when the two agree at every index; tests/test_stage_input_rule.py and
tests/test_gpu_stage_inputs.py use this module to show that they do on what it admits and do not on what it refuses."""
import numpy as np

NEARBY_SCAN = 2.5
K_MAX_RINGS = 64
INT_MAX = 2 ** 31 - 1


def lines_of(cloud):
    """int(intensity) as C++ converts a float (truncation towards zero); the values must be finite and fit an int."""
    return np.trunc(np.asarray(cloud, dtype=np.float32)[:, 3].astype(np.float64)).astype(np.int64)


def literal_breaks(L, idx, corner):
    """Index where the upward walk from idx breaks (len(L) if it runs off the end) and where the downward one does (-1), transcribed from
    the reference's loops: the corner walk skips lines on the wrong side of r before its break test, the plane walk does not."""
    r = int(L[idx])
    up, down = len(L), -1
    for j in range(idx + 1, len(L)):
        if corner and int(L[j]) <= r:
            continue
        if int(L[j]) > (r + NEARBY_SCAN):
            up = j
            break
    for j in range(idx - 1, -1, -1):
        if corner and int(L[j]) >= r:
            continue
        if int(L[j]) < (r - NEARBY_SCAN):
            down = j
            break
    return up, down


def stop_tables(L):
    """The device's tables: first / last index of every line in [0, 64) (lines outside are ignored), suffix minimum / prefix maximum."""
    first = np.full(K_MAX_RINGS, INT_MAX, dtype=np.int64)
    last = np.full(K_MAX_RINGS, -1, dtype=np.int64)
    for i, v in enumerate(L):
        if 0 <= v < K_MAX_RINGS:
            first[v] = min(first[v], i)
            last[v] = max(last[v], i)
    suffix_min = np.minimum.accumulate(first[::-1])[::-1]
    prefix_max = np.maximum.accumulate(last)
    return suffix_min, prefix_max


def device_breaks(L, idx, tables):
    """(stop_f, stop_b) the device uses for a walk from idx: stop_f clipped to len(L) like the literal walk's end."""
    suffix_min, prefix_max = tables
    r = int(L[idx])
    f = suffix_min[r + 3] if r + 3 < K_MAX_RINGS else INT_MAX
    b = prefix_max[r - 3] if r - 3 >= 0 else -1
    return min(int(f), len(L)), int(b)


def walk_mismatches(L, indices=None):
    """Indices (with their lines in [0, 64)) where the device's stops differ from the literal walk's breaks, corner or plane walk; all
    indices, or those of `indices`."""
    L = np.asarray(L, dtype=np.int64)
    tables = stop_tables(L)
    bad = []
    for idx in (range(len(L)) if indices is None else indices):
        if not 0 <= L[idx] < K_MAX_RINGS:
            continue
        dev = device_breaks(L, idx, tables)
        if literal_breaks(L, idx, True) != dev or literal_breaks(L, idx, False) != dev:
            bad.append(idx)
    return bad


def rule_fault(cloud, walked):
    """numpy statement of the admission rule: (rule, first point) with rule 0 ok, 1 non-finite, 2 line outside [0, 64), 3 a line more than
    2 below the largest earlier one."""
    c = np.asarray(cloud, dtype=np.float32).reshape(-1, 4)
    finite = np.isfinite(c).all(axis=1)
    highest = None
    for i in range(c.shape[0]):
        if not finite[i]:
            return 1, i
        if not walked:
            continue
        v = float(c[i, 3])
        if not -1.0 < v < 64.0:
            return 2, i
        L = int(v)   # truncation towards zero, like C++
        if highest is not None and highest - L > 2:
            return 3, i
        highest = L if highest is None else max(highest, L)
    return 0, -1
