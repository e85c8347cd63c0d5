"""Inputs shared by tests/test_surf_stack_config.py (CPU) and tests/test_gpu_surf_stack.py: the street drive whose surf stack exceeds the
default capacity, and a constructed laserCloudSurfLast of an exact number of voxels."""
import numpy as np

LEAF = 0.2                      # mapping_line_resolution = mapping_plane_resolution of every case here
STREET = dict(n_rings=64, n_azimuth=2048, n_sweeps=6)
LATTICE_SHAPE = (64, 256)       # the golden shape the lattice case drives its ordinary sweeps with
LATTICE_SWEEP = 2               # the sweep whose laserCloudSurfLast is replaced


def ground_lattice(synth, seq, n, k=LATTICE_SWEEP, spacing=0.45, side=256, seed=3):
    """n points of a jittered lattice (`spacing` apart, jitter +-0.1 m, so no two share a 0.2 m voxel) on the ground plane the sweep sees,
    centred under the sensor of sweep k and expressed in that sweep's sensor frame (ground truth pose): after scan-to-map they lie on the
    ground the earlier sweeps mapped, and the ones near the sensor find five map neighbours within 1 m.  Row-major over (side + 1) x side
    cells, so the first side * side points are a square and n = side * side + 1 adds one cell of the next row.  The ground alone gives
    thousands of accepted plane factors (5 978 in outer round 0 at n = 65 536); wall planes were not needed for the bound of 1 000."""
    assert n <= (side + 1) * side
    rng = np.random.default_rng(seed)
    R, t = seq.pose(k)
    ij = np.stack(np.meshgrid(np.arange(side + 1), np.arange(side), indexing="ij"), -1).reshape(-1, 2)[:n].astype(np.float64)
    xy = (ij - side / 2) * spacing + rng.uniform(-0.1, 0.1, (n, 2)) + t[None, :2]
    pw = np.concatenate([xy, synth.GROUND_Z + rng.normal(0.0, 0.01, (n, 1))], axis=1)
    out = np.zeros((n, 4), np.float32)
    out[:, :3] = ((pw - t[None, :]) @ R).astype(np.float32)
    return out
