"""GPU: place recognition — descriptors, match records and database bytes against the NumPy model of tests/place_model.py, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import place_model as model

pytestmark = pytest.mark.gpu

GEOMETRIES = [(20, 60), (1, 1), (3, 4), (5, 64), (7, 65), (32, 120)]   # one and two passes of lanes, odd and even W, a single sector


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings a HIP runtime of its own: up before this module's first handle (tests/test_gpu_host_input.py); the device forms take tensors."""
    import torch
    torch.zeros(1).cuda()


def enabled(vl, R=20, S=60, capacity=512, **kw):
    h = vl.Handle(0, scan_line=16, with_mapping=0)
    h.place_enable(n_ring=R, n_sector=S, capacity=capacity, **kw)
    return h, model.Geometry(R, S, **dict(dict(min_range=h.cfg.minimum_range), **kw))


def bits(v):
    return np.ascontiguousarray(v).tobytes()


def adversarial(g):
    """Points on every threshold of the specification."""
    f = np.float32
    below = lambda v: np.nextafter(f(v), f(-np.inf))
    above = lambda v: np.nextafter(f(v), f(np.inf))
    e = [f(f(i) * g.w) for i in range(1, g.R)]   # x = e, y = 0: r2 == edge2[i] exactly
    xs = [g.min_range, below(g.min_range), above(g.min_range), g.max_range, below(g.max_range), below(below(g.max_range))]
    for v in e:
        xs += [v, below(v), above(v)]
    pts = []
    for x in xs:
        for sx in (1.0, -1.0):
            for y in (0.0, -0.0):   # y = +-0 with x < 0: atan2f = +-pi, both ends of the sector range and the S - 1 clamp
                pts.append([sx * x, y, 0.5, 0.0])
    pts += [[0.0, float(x), 0.5, 0.0] for x in xs[:6]] + [[0.0, -float(x), 0.5, 0.0] for x in xs[:6]]
    for a in np.linspace(-np.pi, np.pi, 4 * g.S + 1):   # sector boundaries (as near as f64 -> f32 puts them)
        pts.append([10.0 * np.cos(a), 10.0 * np.sin(a), 0.25, 0.0])
    zs = [g.z_min, below(g.z_min), f(g.z_min - f(1.0)), f(g.z_min + f(254.0) * g.z_step), f(g.z_min + f(255.0) * g.z_step), f(g.z_min + f(300.0) * g.z_step), f(-3.0e38),
          f(3.0e38), f(g.z_min + f(7.0) * g.z_step), below(f(g.z_min + f(7.0) * g.z_step))]
    pts += [[3.0 + 0.5 * k, 1.0 + k, float(z), 0.0] for k, z in enumerate(zs)]
    for c in range(3):
        for bad in (np.nan, np.inf, -np.inf):
            p = [5.0, 5.0, 1.0, 0.0]
            p[c] = bad
            pts.append(p)
    pts += [[3.0e38, 1.0, 0.0, 0.0], [1.0e-30, 1.0e-30, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [7.0, 7.0, 0.0, np.nan]]   # r2 overflows; r2 underflows; the origin; w is ignored
    return np.array(pts, np.float32)


def random_rows(rng, g, n):
    b = np.zeros((n, g.S, 4 * g.W), np.uint8)
    b[:, :, :g.R] = rng.integers(0, 256, (n, g.S, g.R))
    b[:, :, :g.R] *= rng.integers(0, 2, (n, g.S, g.R)).astype(np.uint8)   # about half the cells empty
    return b.reshape(n, -1).view("<u4").astype(np.uint32)


@pytest.mark.parametrize("R,S", GEOMETRIES)
def test_descriptors_equal_the_model(vl, sweeps, R, S):
    import torch
    h, g = enabled(vl, R, S)
    sweep = sweeps(16, 256, 0)
    rng = np.random.default_rng(11)
    clouds = [sweep, adversarial(g)] + [sweep[rng.permutation(sweep.shape[0])[:n]] for n in (0, 1, 63, 65, 257)]
    for c in clouds:
        want, winfo = model.describe(c, g)
        got, info = h.place_describe(c)
        assert info == winfo, (R, S, c.shape, info, winfo)
        assert bits(got) == bits(want), (R, S, c.shape, np.flatnonzero(got != want)[:8])
        assert bits(h.place_describe(c)[0]) == bits(got)   # the scratch is cleared between calls
    # the device form, and a second geometry of the filters
    t = torch.from_numpy(sweep).cuda()
    d, i2 = torch.zeros(g.words, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    h.place_describe_device(t, d, i2)
    h.sync()
    want, winfo = model.describe(sweep, g)
    assert bits(d.cpu().numpy().view(np.uint32)) == bits(want) and tuple(i2.cpu().tolist()) == winfo
    h.close()
    h2, g2 = enabled(vl, R, S, min_range=2.5, max_range=31.0, z_min=-1.25, z_step=0.125)
    for c in (sweep, adversarial(g2)):
        want, winfo = model.describe(c, g2)
        got, info = h2.place_describe(c)
        assert info == winfo and bits(got) == bits(want), (R, S, info, winfo)
    h2.close()


@pytest.mark.parametrize("R,S", GEOMETRIES)
def test_match_records_equal_the_model(vl, R, S):
    h, g = enabled(vl, R, S)
    rng = np.random.default_rng(100 * R + S)
    rows = random_rows(rng, g, 300)
    rows[40] = rows[7]                                         # duplicate rows: the smaller row ranks first
    rows[64] = rows[7]
    const = np.tile(random_rows(rng, g, 1).reshape(g.S, g.W)[:1], (g.S, 1)).reshape(-1)   # constant across sectors: shift 0 wins the tie
    rows[1] = const
    tags = rng.integers(-5, 1 << 30, 300).astype(np.int32)
    unpacked = rows.view(np.uint8).reshape(300, g.S, 4 * g.W)[:, :, :g.R]
    turned = np.zeros((g.S, 4 * g.W), np.uint8)
    turned[:, :g.R] = np.roll(unpacked[30], 3 % g.S, axis=0)   # row 30 turned by +3 sectors
    queries = [rows[7], const, random_rows(rng, g, 1)[0], np.zeros(g.words, np.uint32), turned.reshape(-1).view("<u4").astype(np.uint32)]
    # an empty database
    rec = h.place_query_descriptor(queries[0], k=3)
    assert rec["row"].tolist() == [-1, -1, -1] and bits(rec) == bits(model.query(queries[0], rows[:0], tags[:0], g, k=3))
    matched = [model.match_all(q, rows, g) for q in queries]   # a row's distance does not depend on the rows behind it: computed once
    have = 0
    for count in (1, 2, 63, 64, 65, 300):
        h.place_load(rows[have:count], tags[have:count])
        have = count
        assert h.place_count() == count
        for q, mq in zip(queries, matched):
            for k, ex in ((8, 0), (1, 0), (3, 1), (8, count), (2, count + 1), (8, max(count - 2, 0))):   # k larger than the row count included
                want = model.records(mq, tags, count, k=k, exclude_last=ex)
                got = h.place_query_descriptor(q, k=k, exclude_last=ex)
                assert bits(got) == bits(want), (R, S, count, k, ex, got, want)
        assert bits(h.place_query_descriptor(queries[2], k=8)) == bits(h.place_query_descriptor(queries[2], k=8))   # the same query twice
    rec = h.place_query_descriptor(rows[7], k=4)
    if R * S >= 12:   # (with a handful of cells other rows can be equal too)
        assert rec["row"][:3].tolist() == [7, 40, 64] and rec["dist"][:3].tolist() == [0, 0, 0]
    rec = h.place_query_descriptor(queries[4], k=1)[0]
    if R * S >= 12 and np.count_nonzero(unpacked[30]) > 2:   # the yaw convention: content turned by +m sectors gives shift m
        assert (rec["row"], rec["shift"], rec["dist"]) == (30, 3 % S, 0), rec
    # database bytes: what went in comes out, with the cells counted
    d, t, info = h.place_get()
    assert bits(d) == bits(rows) and bits(t) == bits(tags) and info[:, 0].tolist() == [-1] * 300
    assert info[:, 1].tolist() == np.count_nonzero(unpacked, axis=(1, 2)).tolist()
    # a pad byte that is not zero is refused, and the database stays as it is
    if 4 * g.W > R:
        bad = rows[:2].copy()
        bad[1, g.W - 1] |= np.uint32(1 << 31)
        for call in (lambda: h.place_load(bad, tags[:2]), lambda: h.place_query_descriptor(bad[1])):
            with pytest.raises(vl.VloamError) as e:
                call()
            assert e.value.status == vl.ERR_INVALID and "pad byte" in str(e.value)
        assert h.place_count() == 300
    # a get / load round trip into a second handle answers identically
    h2, _ = enabled(vl, R, S)
    h2.place_load(d, t)
    for q in queries:
        assert bits(h2.place_query_descriptor(q, k=8, exclude_last=5)) == bits(h.place_query_descriptor(q, k=8, exclude_last=5))
    h.close()
    h2.close()


def test_add_get_describe_query_and_capacity(vl, sweeps):
    import torch
    h, g = enabled(vl, capacity=4)
    clouds = [sweeps(16, 256, k) for k in range(5)]
    descs = [h.place_describe(c) for c in clouds]
    assert h.place_count() == 0
    assert [h.place_add(c, 100 + k) for k, c in enumerate(clouds[:3])] == [0, 1, 2]
    assert h.place_add_device(torch.from_numpy(clouds[3]).cuda(), 103) == 3 and h.place_count() == 4
    d, t, info = h.place_get()
    assert t.tolist() == [100, 101, 102, 103]
    for k in range(4):   # place_get after place_add equals place_describe, and the model
        assert bits(d[k]) == bits(descs[k][0]) == bits(model.describe(clouds[k], g)[0]) and tuple(info[k]) == descs[k][1]
    for add in (lambda: h.place_add(clouds[4], 104), lambda: h.place_add_device(torch.from_numpy(clouds[4]).cuda(), 104), lambda: h.place_load(d[:1], t[:1])):
        with pytest.raises(vl.VloamError) as e:   # the fifth row
            add()
        assert e.value.status == vl.ERR_CAPACITY
    d2, t2, info2 = h.place_get()
    assert h.place_count() == 4 and bits(d2) == bits(d) and bits(t2) == bits(t) and bits(info2) == bits(info)
    assert bits(h.place_get(1, 2)[0]) == bits(d[1:3]) and h.place_get(4, 0)[0].shape[0] == 0
    with pytest.raises(vl.VloamError) as e:
        h.place_get(3, 2)
    assert e.value.status == vl.ERR_INVALID
    # queries by cloud: host and device form, against the model
    out = torch.zeros(3 * 32, dtype=torch.uint8, device="cuda")
    for k, c in enumerate(clouds):
        want = model.query(model.describe(c, g)[0], d, t, g, k=3, exclude_last=1)
        got = h.place_query(c, k=3, exclude_last=1)
        h.place_query_device(torch.from_numpy(c).cuda(), out, k=3, exclude_last=1)
        h.sync()
        assert bits(got) == bits(want) == bits(out.cpu().numpy()), (k, got, want)
        if k < 3:
            assert (got[0]["row"], got[0]["tag"], got[0]["shift"], got[0]["dist"]) == (k, 100 + k, 0, 0)
    # once per handle; not on a batched handle
    with pytest.raises(vl.VloamError) as e:
        h.place_enable()
    assert e.value.status == vl.ERR_ORDER
    h.close()
    hb = vl.Handle(0, n_sessions=2, scan_line=16, with_mapping=0)
    with pytest.raises(vl.VloamError) as e:
        hb.place_enable()
    assert e.value.status == vl.ERR_INVALID and "not offered" in str(e.value)
    hb.close()


def test_every_call_on_a_handle_that_was_not_enabled_is_an_order_error(vl):
    h = vl.Handle(0, scan_line=16, with_mapping=0)
    L = vl.lib()
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    cloud, desc, info, tags = np.ones((5, 4), np.float32), np.zeros(300, np.uint32), np.zeros(2, np.int32), np.zeros(1, np.int32)
    out, q = np.zeros(8, vl.PLACE_MATCH_DTYPE), vl.PlaceQueryOptions(16, 1, 0, 0)
    row, cnt = C.c_int(0), C.c_int(0)
    calls = [("vloam_place_describe", (P(cloud), 5, P(desc), P(info))), ("vloam_place_describe_device", (P(cloud), 5, P(desc), P(info))),
             ("vloam_place_add", (P(cloud), 5, 1, C.byref(row))), ("vloam_place_add_device", (P(cloud), 5, 1, C.byref(row))),
             ("vloam_place_count", (C.byref(cnt),)), ("vloam_place_get", (0, 1, P(desc), P(tags), P(info))), ("vloam_place_load", (P(desc), P(tags), 1)),
             ("vloam_place_query", (C.byref(q), P(cloud), 5, P(out))), ("vloam_place_query_device", (C.byref(q), P(cloud), 5, P(out))),
             ("vloam_place_query_descriptor", (C.byref(q), P(desc), P(out)))]
    for name, args in calls:
        assert getattr(L, name)(h.h, *args) == vl.ERR_ORDER, name
        assert L.vloam_last_error().startswith(name.encode() + b": vloam_place_enable has not been called"), name
    h.close()


def test_a_turned_sweep_matches_as_the_model_says(vl, sweeps):
    h, g = enabled(vl)
    clouds = [sweeps(16, 256, k) for k in (3, 0, 5)]
    for k, c in enumerate(clouds):
        h.place_add(c, k)
    d, t, _ = h.place_get()
    base = clouds[1].astype(np.float64)
    for m in (1, 7, g.S - 1):
        a = m * 2.0 * np.pi / g.S
        rot = base.copy()
        rot[:, 0], rot[:, 1] = np.cos(a) * base[:, 0] - np.sin(a) * base[:, 1], np.sin(a) * base[:, 0] + np.cos(a) * base[:, 1]
        rot = rot.astype(np.float32)
        want = model.query(model.describe(rot, g)[0], d, t, g, k=3)   # the model, not an assumed distance of 0, is the expectation
        got = h.place_query(rot, k=3)
        print("turned by %d sectors: row %d shift %d dist %d (runner-up %d)" % (m, got[0]["row"], got[0]["shift"], got[0]["dist"], got[1]["dist"]))
        assert bits(got) == bits(want), (m, got, want)
        assert got[0]["row"] == 1 and got[0]["shift"] == m   # the yaw convention on real content
    h.close()


def test_the_sequence_is_untouched(vl, sweeps):
    hs = [vl.Handle(0, scan_line=16, with_mapping=1) for _ in range(2)]
    hs[0].place_enable()
    for k in range(6):
        c = sweeps(16, 256, k)
        for j, h in enumerate(hs):
            h.process_scan(c)
            if j == 0:
                assert h.place_add(c, k) == k
    for h in hs:
        h.sync()
    assert hs[0].place_count() == 6
    assert bits(hs[0].trajectory()) == bits(hs[1].trajectory()) and hs[0].frame_count() == 6
    assert bits(hs[0].get_map()) == bits(hs[1].get_map()) and hs[0].get_map().shape[0] > 0
    for h in hs:
        h.close()
