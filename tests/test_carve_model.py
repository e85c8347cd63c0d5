"""CPU: the NumPy statement of vloam_map_carve (tests/carve_model.py) on hand-made scenes — what the rule removes and what it keeps.  The
device is compared with this model bit for bit in tests/test_gpu_carve.py."""
import numpy as np

import carve_model as cm

OPT = dict(rows=16, cols=256, elev_min_deg=-16.0, elev_max_deg=16.0, min_range=1.0, max_range=80.0, range_res=0.05, margin=0.5)
IDENT = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
GROUND_Z = -1.73


def beams():
    """(elevation, azimuth) [16, 256] of one ray through every pixel centre."""
    el = np.deg2rad(-16.0 + 2.0 * (np.arange(16) + 0.5))
    az = -np.pi + (np.arange(256) + 0.5) * 2.0 * np.pi / 256
    return np.meshgrid(el, az, indexing="ij")


def sweep_of(range_fn):
    """float32 [4096, 4] sweep: range_fn(el, az) -> range per ray (NaN / inf: no return)."""
    el, az = beams()
    r = range_fn(el, az)
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], -1)
    out = np.zeros((el.size, 4), np.float32)
    with np.errstate(invalid="ignore"):
        out[:, :3] = (d * r[..., None]).reshape(-1, 3).astype(np.float32)
    out[~np.isfinite(out[:, 0]), :3] = np.nan
    return out


def wall_and_ground(el, az):
    """A wall x = 20 m (|azimuth| < 40 degrees, up to 4 m above the sensor) on a ground plane z = -1.73 m."""
    with np.errstate(divide="ignore", invalid="ignore"):
        rw = 20.0 / (np.cos(el) * np.cos(az))
        rg = np.where(el < 0, GROUND_Z / np.sin(el), np.inf)
    rw = np.where((np.abs(az) < np.deg2rad(40.0)) & (rw * np.sin(el) < 4.0), rw, np.inf)
    r = np.minimum(rw, rg)
    return np.where(r <= 80.0, r, np.nan)


def run(points, sweeps, poses=None, **kw):
    o = dict(OPT)
    o.update(kw)
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    removed, cnt = cm.carve(pts, sweeps, poses or [IDENT] * len(sweeps), **o)
    return removed, cnt


def test_front_of_wall_goes_wall_and_behind_stay():
    s = sweep_of(wall_and_ground)
    pts = [[10.0, 0.2, 0.1],     # in front of the wall: the beam through it returned from 20 m
           [20.0, 0.3, 0.1],     # on the wall
           [20.3, -2.0, 0.5],    # on the wall, inside the margin
           [30.0, 0.2, 0.1],     # behind it
           [0.2, 10.0, 2.0]]     # where the sweep has no return at all (no wall at 90 degrees, above the ground rows)
    removed, cnt = run(pts, [s])
    assert removed.tolist() == [True, False, False, False, False]
    assert cnt == dict(examined=5, in_view=5, seen_through=1, confirmed=2, removed=1)
    G = cm.Geom(**OPT)
    view, through, confirm = cm.votes(G, np.asarray(pts, np.float32), [cm.range_image(G, s)], [IDENT])
    assert view.tolist() == [1, 1, 1, 1, 1] and through.tolist() == [1, 0, 0, 0, 0] and confirm.tolist() == [0, 1, 1, 0, 0]
    ok, row, col, _ = cm.project(G, np.asarray(pts[4:], np.float32))
    assert ok[0] and cm.range_image(G, s)[row[0], col[0]] == cm.EMPTY


def test_ground_at_grazing_incidence_stays():
    """A ground point between two rings' footprints: its pixel's beam returns from 8 m further out, the ring below from nearer — the
    neighbourhood minimum keeps it where the centre pixel alone would have removed it."""
    s = sweep_of(wall_and_ground)
    G = cm.Geom(**OPT)
    img = cm.range_image(G, s)
    strip = np.array([[25.0 * np.cos(a), 25.0 * np.sin(a), GROUND_Z] for a in np.deg2rad([60.0, 75.0, 90.0, 120.0, -100.0])], np.float32)
    ok, row, col, q = cm.project(G, strip)
    assert ok.all()
    cen = img[row, col].astype(np.int64)
    assert (cen != int(cm.EMPTY)).all() and (q + G.margin_q < cen).all()          # the centre pixel alone sees through every one of them
    assert (img[row - 1, col].astype(np.int64) < q).all()                         # the ring below returned from nearer
    removed, cnt = run(strip, [s])
    assert not removed.any() and cnt["seen_through"] == 0 and cnt["confirmed"] == 0 and cnt["in_view"] == 5


def test_columns_wrap_at_pi():
    G = cm.Geom(**OPT)
    # azimuth exactly +pi (y = +0, x < 0) is column `cols`, which is column 0; just below +pi is the last column, just above -pi the first
    ok, row, col, _ = cm.project(G, np.array([[-10.0, 0.0, 0.0], [-10.0, 1e-3, 0.0], [-10.0, -1e-3, 0.0]], np.float32))
    assert ok.all() and col.tolist() == [0, 255, 0]

    def far_last_near_first(el, az):   # behind the sensor: 30 m in the last column, 5 m in the first, nothing else
        c = np.floor((az + np.pi) / (2 * np.pi) * 256)
        return np.where(c == 255, 30.02, np.where(c == 0, 5.02, np.nan))

    s = sweep_of(far_last_near_first)
    cand = np.array([[-10.0, 0.12, 0.1]], np.float32)     # 10 m, in the last column: its beam returned from 30 m ...
    ok, row, col, q = cm.project(G, cand)
    assert col[0] == 255 and cm.range_image(G, s)[row[0], 255] == 600 and cm.range_image(G, s)[row[0], 0] == 100
    removed, cnt = run(cand, [s])
    assert not removed[0] and cnt["seen_through"] == 0   # ... but the neighbour across the seam returned from 5 m

    def far_both(el, az):
        c = np.floor((az + np.pi) / (2 * np.pi) * 256)
        return np.where((c >= 254) | (c <= 1), 30.0, np.nan)

    removed, cnt = run(cand, [sweep_of(far_both)])
    assert removed[0] and cnt["seen_through"] == 1


def test_min_votes_and_confirmation_over_sweeps():
    s = sweep_of(wall_and_ground)
    blind = sweep_of(lambda el, az: np.full(el.shape, np.nan))
    pts = [[10.0, 0.2, 0.1]]
    assert run(pts, [s])[0][0]
    removed, cnt = run(pts, [s, blind], min_votes=2)
    assert not removed[0] and cnt["seen_through"] == 1 and cnt["removed"] == 0    # one sweep that sees through is not two votes
    assert run(pts, [s, s], min_votes=2)[0][0]
    # a sweep that still sees the object protects it, however many see through

    def with_object(el, az):
        r = wall_and_ground(el, az)
        return np.where((np.abs(az) < np.deg2rad(3.0)) & (np.abs(el) < np.deg2rad(3.0)), 10.0, r)

    removed, cnt = run(pts, [s, s, sweep_of(with_object)])
    assert not removed[0] and cnt["seen_through"] == 1 and cnt["confirmed"] == 1


def test_pose_moves_the_candidate_into_the_sensor_frame():
    s = sweep_of(wall_and_ground)
    yaw = np.deg2rad(30.0)
    pose = [0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2), 5.0, -2.0, 0.5]
    R, t = cm.pose_matrix(pose)
    sensor_pts = np.array([[10.0, 0.2, 0.1], [20.0, 0.3, 0.1]])
    removed, _ = run((sensor_pts @ R.T + t).astype(np.float32), [s], poses=[pose])
    assert removed.tolist() == [True, False]
    back = cm.to_sensor((sensor_pts @ R.T + t).astype(np.float32), pose)
    assert np.abs(back - sensor_pts).max() < 1e-5


def test_out_of_range_and_non_finite_points_are_ignored():
    G = cm.Geom(**OPT)
    pts = np.array([[0.5, 0.0, 0.0], [90.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [5.0, 0.0, 5.0], [1.0, 0.0, 0.0], [80.0, 0.0, 0.0]], np.float32)
    ok, _, _, q = cm.project(G, pts)
    assert ok.tolist() == [False, False, False, False, True, True] and q[4:].tolist() == [20, 1600]
    one = np.zeros((1, 4), np.float32)
    one[0, :3] = [7.0, 0.0, 0.0]
    img = cm.range_image(cm.Geom(rows=1, cols=4, elev_min_deg=-16.0, elev_max_deg=16.0), one)
    assert img.shape == (1, 4) and img[0].tolist() == [int(cm.EMPTY), int(cm.EMPTY), 140, int(cm.EMPTY)]
