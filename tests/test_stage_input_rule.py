"""CPU: the admission rule of substituted stage clouds (csrc/stage_input_check.h) against the reference's walk (tests/stage_walk_model.py).

vloam_set_odometry_input refuses a cloud with a non-finite value and, in the two less-clouds the next sweep's odometry walks by scan line,
a line outside [0, 64) or a line more than 2 below an earlier one.  Here the header is compiled on its own with g++ and run over a few
thousand seeded line sequences.  What it admits: at every index the device's walk-stop tables equal the break indices of the reference's
literal corner and plane walks.  What it refuses for its order: some index where they differ, i.e. a cloud the device would walk
differently.  Its verdict and the point it names equal the numpy statement of the rule."""
import os
import struct
import subprocess

import numpy as np
import pytest

import stage_walk_model as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stage_check") / "stage_input_check")
    subprocess.run(["g++", "-O1", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "vloam-cmu-16833_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "stage_input_check.cpp"), "-o", exe], check=True)

    def run(cases):
        path = exe + ".in"
        with open(path, "wb") as f:
            f.write(struct.pack("<i", len(cases)))
            for cloud, walked in cases:
                c = np.ascontiguousarray(cloud, dtype=np.float32).reshape(-1, 4)
                f.write(struct.pack("<ii", c.shape[0], int(walked)))
                f.write(c.tobytes())
        out = subprocess.run([exe, path], capture_output=True, text=True, check=True).stdout.split("\n")
        return [tuple(int(v) for v in ln.split()) for ln in out if ln]
    return run


def sorted_cloud(rng, n_max=48):
    """Scan registration's order: lines ascending, intensity = r + 0.1 relTime with the r / r - 1 jitter of int(intensity)."""
    lines = np.sort(rng.choice(64, size=rng.integers(1, 9), replace=False))
    counts = rng.integers(1, 7, size=lines.size)
    r = np.repeat(lines, counts)[:n_max]
    frac = rng.uniform(-0.05, 0.15, size=r.size)
    inten = (r + frac).astype(np.float32)
    xyz = rng.normal(0, 10, size=(r.size, 3)).astype(np.float32)
    return np.column_stack([xyz, inten]).astype(np.float32)


def shuffle_within_lines(rng, c):
    L = wm.lines_of(c)
    key = np.lexsort((rng.random(L.size), L))
    return c[key]


def windows_of_three_reversed(c):
    L = wm.lines_of(c)
    return c[np.lexsort((np.arange(L.size), 2 - L % 3, L // 3))]


def local_swaps(rng, c):
    c = c.copy()
    for _ in range(rng.integers(1, 4)):
        if c.shape[0] < 2:
            break
        i = rng.integers(0, c.shape[0] - 1)
        j = min(c.shape[0] - 1, i + rng.integers(1, 12))
        c[[i, j]] = c[[j, i]]
    return c


def one_inversion(rng, c):
    """One point moved below the largest earlier line by 3 or more."""
    c = c.copy()
    L = wm.lines_of(c)
    cand = [i for i in range(1, L.size) if L[:i].max() >= 3]
    if not cand:
        return None
    i = int(rng.choice(cand))
    top = int(L[:i].max())
    c[i, 3] = np.float32(rng.integers(0, top - 2) + rng.uniform(0.0, 0.99))
    return c


def out_of_range(rng, c):
    c = c.copy()
    i = rng.integers(0, c.shape[0])
    c[i, 3] = np.float32(rng.choice([64.0, 64.02, 70.5, -1.0, -1.02, -3.5, 1e30, -1e30, 2.2e9]))
    return c


def non_finite(rng, c):
    c = c.copy()
    c[rng.integers(0, c.shape[0]), rng.integers(0, 4)] = rng.choice([np.nan, np.inf, -np.inf])
    return c


def test_rule_equals_the_reference_walk_on_seeded_sequences(checker):
    rng = np.random.default_rng(20261016)
    cases, kinds = [], []
    for _ in range(600):
        c = sorted_cloud(rng)
        variants = [("sorted", c), ("shuffled", shuffle_within_lines(rng, c)), ("windows", windows_of_three_reversed(c)),
                    ("swaps", local_swaps(rng, c)), ("inversion", one_inversion(rng, c)), ("range", out_of_range(rng, c)),
                    ("nonfinite", non_finite(rng, c))]
        for kind, v in variants:
            if v is not None:
                cases.append((v, True))
                kinds.append(kind)
        cases.append((non_finite(rng, c) if rng.random() < 0.5 else out_of_range(rng, c), False))   # a cloud that is not walked
        kinds.append("unwalked")
    # the edges of rule 2 and 3 spelled out
    edge = np.array([[1, 2, 3, -0.99], [1, 2, 3, 2.0], [1, 2, 3, 0.5], [1, 2, 3, 63.99], [1, 2, 3, 61.0]], np.float32)   # inversions of exactly 2
    for c, k in ((edge, "edge_ok"), (edge[[0, 2, 4]], "edge_ok"), (np.array([[0, 0, 0, 5.0], [0, 0, 0, 2.99]], np.float32), "edge_bad"),
                 (np.zeros((0, 4), np.float32), "empty"), (np.array([[0, 0, 0, 64.0]], np.float32), "edge_bad")):
        cases.append((c, True))
        kinds.append(k)
    got = checker(cases)
    assert len(got) == len(cases)
    seen = {}
    for (cloud, walked), kind, (rule, point, _) in zip(cases, kinds, got):
        assert (rule, point) == wm.rule_fault(cloud, walked), (kind, cloud)
        seen[(kind, rule)] = seen.get((kind, rule), 0) + 1
        if not walked:
            assert rule in (0, 1)
            continue
        if rule == 0:
            assert wm.walk_mismatches(wm.lines_of(cloud)) == [], (kind, cloud)
        elif rule == 3:
            assert wm.walk_mismatches(wm.lines_of(cloud)), (kind, cloud)
    # every admissible family is admitted, every refused one refused
    for kind in ("sorted", "shuffled", "windows", "empty", "edge_ok"):
        assert all(r == 0 for (k, r) in seen if k == kind), kind
    assert set(r for (k, r) in seen if k == "inversion") == {3}
    assert set(r for (k, r) in seen if k == "range") == {2}
    assert set(r for (k, r) in seen if k == "nonfinite") == {1}
    assert set(r for (k, r) in seen if k == "edge_bad") == {2, 3}
    assert seen.get(("swaps", 0), 0) > 20 and seen.get(("swaps", 3), 0) > 20, "local swaps land on both sides of the rule"
    assert seen.get(("windows", 0), 0) > 500


def test_windows_of_three_are_the_largest_admitted_inversion():
    """Lines reversed in windows of three: the largest inversion is exactly 2 and every walk breaks where the device's stops say; one more
    line of distance (windows of four) and the walks part."""
    L = np.repeat(np.arange(12), 3)
    w3 = L[np.lexsort((np.arange(L.size), 2 - L % 3, L // 3))]
    w4 = L[np.lexsort((np.arange(L.size), 3 - L % 4, L // 4))]
    inv = lambda s: max(int(s[:i].max()) - int(s[i]) for i in range(1, s.size))
    assert inv(w3) == 2 and wm.walk_mismatches(w3) == []
    assert inv(w4) == 3 and wm.walk_mismatches(w4) != []
