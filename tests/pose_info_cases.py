"""Shared by tests/test_gpu_pose_info.py: the oracle's factor sets of the LAST outer round of a sweep's odometry / mapping as rows for
orc.solve (oracle/orc_capi.cpp: orc_solve), and the oracle's J^T J / cost of such a set at a given pose.  The constructions are those of
tests/test_gpu_laser_odometry.py (correspondence indices into the sweep's sharp / flat clouds and the previous sweep's CornerLast / SurfLast)
and tests/test_gpu_laser_mapping.py (stack indices + the line / plane fitted through the five nearest map points)."""
import numpy as np


class OracleRun:
    """Drives the oracle sweep by sweep and keeps, per sweep, the orc.solve rows of the last odometry round and of the last mapping round
    (None where the stage did not solve) and the oracle's own poses."""

    def __init__(self, orc, **kw):
        self.orc = orc
        self.o = orc.Oracle(**kw)
        self.corner_last = self.surf_last = None
        self.lo_rows, self.map_rows, self.lo_x, self.map_x = [], [], [], []

    def process(self, cloud):
        o = self.o
        assert o.process(cloud) == 0
        lo = mp = None
        if o.lo_num_outer() == 2:
            sharp, flat = o.cloud(1).astype(np.float64), o.cloud(3).astype(np.float64)
            cl, sl = self.corner_last.astype(np.float64), self.surf_last.astype(np.float64)
            c, p = o.lo_corr(1)
            lo = [[0, *sharp[i, :3], *cl[a, :3], *cl[b, :3]] for i, a, b in c] + \
                 [[1, *flat[i, :3], *sl[j, :3], *sl[l, :3], *sl[m, :3]] for i, j, l, m in p]
            lo = (lo, c.shape[0], p.shape[0])
        if o.map_num_outer() == 2:
            cs, ss = o.cloud(7).astype(np.float64), o.cloud(8).astype(np.float64)
            ci, cab, si, spl = o.map_factors(1)
            mp = [[0, *cs[i, :3], *cab[k]] for k, i in enumerate(ci)] + [[2, *ss[i, :3], *spl[k]] for k, i in enumerate(si)]
            mp = (mp, ci.size, si.size)
        self.lo_rows.append(lo)
        self.map_rows.append(mp)
        _, _, ql, tl = o.lo_pose()
        self.lo_x.append(np.concatenate([ql, tl]))
        q, t, _, _ = o.map_pose()
        self.map_x.append(np.concatenate([q, t]))
        self.corner_last, self.surf_last = o.cloud(5).copy(), o.cloud(6).copy()   # laserCloudCornerLast / laserCloudSurfLast for the next sweep
        return lo, mp

    def matrix(self, rows, x):
        """(H, cost) of the factor set at x = (q xyzw, t): orc_solve's H0 and initial cost, no iteration."""
        s = self.orc.solve(rows[0], x[:4], x[4:], quaternion=True, huber_a=0.1, max_iters=0)
        return s["H0"], s["initial_cost"]


def rel_err(H_dev, H_orc):
    """The norm of tests/test_gpu_laser_odometry.py:34-35."""
    scale = np.sqrt(np.outer(np.diag(H_orc), np.diag(H_orc))) + 1e-30
    return float(np.max(np.abs(H_dev - H_orc) / scale))
