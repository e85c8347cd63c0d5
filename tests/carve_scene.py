"""The scene of the map clean-up tests (tests/test_carve_scene.py on the CPU oracle's map, tests/test_gpu_carve.py on the device's): seven
16 x 256 sweeps of the synthetic drive, 1 m apart, with a PHANTOM box — 2 m deep, 4 m wide, ground to 0.8 m above the sensor, 10 - 12 m ahead
of the first pose, about 200 returns per sweep — cast into sweeps 0 and 1 only.  Sweeps 0 - 4 build the map, sweeps 3 and 4 (which look through
where the box was) carve it, sweeps 5 and 6 drive on afterwards."""
import numpy as np

RINGS, COLS, N_BUILD, N_ALL = 16, 256, 5, 7
MAX_POINTS = RINGS * COLS
PARAMS = dict(minimum_range=0.3, mapping_line_resolution=0.2, mapping_plane_resolution=0.4, mapping_skip_frame=1)   # loam_velodyne_VLP_16.launch:3-13
PHANTOM_SWEEPS, CARVE_SWEEPS = (0, 1), (3, 4)
# the range image of the 16-line head: one row per beam (beams at -15, -13, .. +15 degrees sit mid-row), one column per firing
CARVE = dict(rows=RINGS, cols=COLS, elev_min_deg=-16.0, elev_max_deg=16.0, min_range=1.0, max_range=80.0, range_res=0.05, margin=0.5)
BOX = np.array([10.0, -2.0, -1.73, 12.0, 2.0, 0.8])   # world frame (== the map frame: the first pose is the origin up to its heave, roll and pitch)
BOX_SLACK = 0.45                                      # a voxel centroid of box returns lies inside the box up to the range noise; one surf leaf of room


def cast_phantom(seq, k, cloud):
    """Sweep k with the returns of BOX: every ray that meets the box before its own return (slab test in the world frame) ends on the box."""
    R, o = seq.pose(k)
    d = seq.dirs @ R.T
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (BOX[None, 0:3] - o[None, :]) / d, (BOX[None, 3:6] - o[None, :]) / d
        tmin, tmax = np.nanmax(np.minimum(t1, t2), axis=1), np.nanmin(np.maximum(t1, t2), axis=1)
        r = np.linalg.norm(cloud[:, :3].astype(np.float64), axis=1)
    hit = (tmax >= tmin) & (tmin > 0) & ~(r <= tmin)    # (a missing return is NaN: the box takes the ray)
    out = cloud.copy()
    out[hit, :3] = (seq.dirs[hit] * tmin[hit, None]).astype(np.float32)
    return out, int(hit.sum())


def build(synth):
    """(sweeps [N_ALL] float32 [4096, 4], returns on the phantom per sweep)."""
    seq = synth.SynthSequence(n_rings=RINGS, n_azimuth=COLS, n_sweeps=N_ALL + 1)
    sweeps, hits = [], []
    for k in range(N_ALL):
        c, n = seq.sweep(k), 0
        if k in PHANTOM_SWEEPS:
            c, n = cast_phantom(seq, k, c)
        sweeps.append(c)
        hits.append(n)
    return sweeps, hits


def in_phantom(points):
    p = np.asarray(points)[:, :3]
    return np.all((p >= BOX[None, 0:3] - BOX_SLACK) & (p <= BOX[None, 3:6] + BOX_SLACK), axis=1)


def sorted_rows(a):
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 4)
    u = a.view(np.uint32)
    return a[np.lexsort((u[:, 3], u[:, 2], u[:, 1], u[:, 0]))]
