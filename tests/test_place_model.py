"""CPU: the NumPy model of the place descriptor (tests/place_model.py) against itself on polar-constructed clouds — points at bin centres, and a
copy whose sector indices are moved by m: shift == m and dist == 0 for every m — and the tie rules of c_api.h."""
import numpy as np
import pytest

import place_model as model


def random_cells(rng, g, n):
    return rng.integers(0, g.S, n), rng.integers(0, g.R, n), rng.integers(0, 255, n)


@pytest.mark.parametrize("R,S", [(20, 60), (3, 4), (7, 65), (1, 1)])
def test_bin_centres_land_in_their_cells_and_a_turn_is_a_shift(R, S):
    g = model.Geometry(R, S)
    rng = np.random.default_rng(R * 1000 + S)
    sec, ring, lev = random_cells(rng, g, 150)
    cloud = model.polar_cloud(sec, ring, lev, g)
    cells, used = model.cells_of(cloud, g)
    want = np.zeros((S, R), np.int32)
    np.maximum.at(want, (sec, ring), (lev + 1).astype(np.int32))
    assert used == 150 and np.array_equal(cells, want)
    desc, info = model.describe(cloud, g)
    assert desc.shape == (S * g.W,) and info == (150, int(np.count_nonzero(want))) and np.array_equal(model.unpack(desc, g), want)
    # pad bytes are zero
    assert not model.pack(cells, g).view(np.uint8).reshape(S, 4 * g.W)[:, R:].any()
    distinct = len({np.roll(want, -m, axis=0).tobytes() for m in range(S)}) == S   # no rotational symmetry in the random cells
    assert distinct or S == 1
    for m in range(S):
        # the query's content is the row's turned by +m sectors
        q_cells, _ = model.cells_of(model.polar_cloud((sec + m) % S, ring, lev, g), g)
        assert np.array_equal(q_cells, np.roll(want, m, axis=0))
        dist, shift = model.best(q_cells, want)
        assert (int(dist), int(shift)) == (0, m), (m, dist, shift)
        rec = model.query(model.pack(q_cells, g), desc[None], [42], g)[0]
        assert (rec["row"], rec["tag"], rec["shift"], rec["dist"]) == (0, 42, m, 0) and rec["n_occupied_query"] == rec["n_occupied_row"] == info[1]


def test_dist_is_the_sum_of_absolute_differences():
    g = model.Geometry(3, 4)
    Q = np.array([[1, 0, 0], [0, 0, 0], [0, 5, 0], [0, 0, 0]])
    D = np.array([[0, 0, 0], [0, 7, 0], [0, 0, 0], [2, 0, 0]])   # Q turned back by one sector, other heights
    assert model.dists(Q, D).tolist() == [15, 3, 15, 15]   # s = 1: |5 - 7| + |1 - 2|
    assert tuple(int(v) for v in model.best(Q, D)) == (3, 1)
    assert g.W == 1 and model.pack(Q, g).tolist() == [1, 0, 5 << 8, 0]


def test_tie_rules():
    g = model.Geometry(5, 8)
    rng = np.random.default_rng(5)
    const = np.tile(rng.integers(1, 256, (1, g.R)), (g.S, 1))   # constant across sectors: every shift gives the same distance
    other = rng.integers(0, 256, (g.S, g.R))
    d = model.dists(other, const)
    assert len(set(d.tolist())) == 1 and int(model.best(other, const)[1]) == 0   # shift 0 wins the tie
    period = np.tile(rng.integers(0, 256, (2, g.R)), (g.S // 2, 1))   # period 2: shifts 0, 2, 4, 6 tie at 0
    assert tuple(int(v) for v in model.best(period, period)) == (0, 0)
    assert tuple(int(v) for v in model.best(np.roll(period, 1, axis=0), period)) == (0, 1)
    # duplicate rows: the smaller row ranks first; then dist ascending
    rows = np.stack([model.pack(a, g) for a in (other, const, other, const)])
    tags = [10, 11, 12, 13]
    rec = model.query(model.pack(const, g), rows, tags, g, k=8)
    assert rec["row"].tolist() == [1, 3, 0, 2, -1, -1, -1, -1] and rec["tag"].tolist() == [11, 13, 10, 12, 0, 0, 0, 0]
    assert rec["dist"][:2].tolist() == [0, 0] and rec["dist"][2] == rec["dist"][3] > 0 and not rec["dist"][4:].any()
    # the youngest rows are skipped; a fully excluded database answers with nothing
    assert model.query(model.pack(const, g), rows, tags, g, k=2, exclude_last=1)["row"].tolist() == [1, 0]
    assert model.query(model.pack(const, g), rows, tags, g, k=2, exclude_last=3)["row"].tolist() == [0, -1]
    for ex in (4, 5):
        assert model.query(model.pack(const, g), rows, tags, g, k=2, exclude_last=ex)["row"].tolist() == [-1, -1]
    assert model.query(model.pack(const, g), np.zeros((0, g.words), np.uint32), [], g, k=3)["row"].tolist() == [-1, -1, -1]


def test_filters_and_clamps():
    g = model.Geometry(4, 4, min_range=1.0, max_range=8.0, z_min=-1.0, z_step=0.5)
    nan, inf = np.nan, np.inf
    pts = np.array([[2, 0.5, 0, 0], [nan, 1, 0, 0], [2, inf, 0, 0], [2, 1, -inf, 0], [0.5, 0, 0, 0], [8, 0, 0, 0], [1, 0.5, -9, 0], [3, 0.5, 1e9, 0],
                    [3.0e38, 3.0e38, 0, 0], [2, 0.5, 3.0e38, 0]], np.float32)
    cells, used = model.cells_of(pts, g)
    # used: points 0, 6 (below z_min: level 1), 7 (above the top level: 255) and 9
    assert used == 4 and cells[2, 1] == 255 and cells[2, 0] == 1 and np.count_nonzero(cells) == 2
