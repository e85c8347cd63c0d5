#!/usr/bin/env python3
"""Place-match probe (seconds): vloam_place_query_descriptor against 10 000 and 100 000 rows of the default geometry (20 rings x 60 sectors, 1 200
bytes a row).  Device time: HIP events around the match + top-k launches, warm, median of repeated launches (vloam_place_time_query); next to it
the call's wall time (copies and synchronisation included), the two bounds of DESIGN.md section 8, and the NumPy model's time on the same inputs.
  python tools/place_probe.py [--rows 10000,100000] [--repeats 50] [--k 8] [--model-rows 100000]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest  # noqa: E402
import place_model as model  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", default="10000,100000")
ap.add_argument("--repeats", type=int, default=50)
ap.add_argument("--warm", type=int, default=10)
ap.add_argument("--k", type=int, default=8)
ap.add_argument("--model-rows", type=int, default=100000, help="the NumPy model runs only for databases up to this many rows (it takes about a minute per 100 000)")
ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM bandwidth for the bound, TB/s (MI355X: 8)")
ap.add_argument("--cus", type=int, default=256)
ap.add_argument("--ghz", type=float, default=2.4)
a = ap.parse_args()
vl = conftest.load_pkg()
g = model.Geometry()
rng = np.random.default_rng(7)


def random_rows(n):
    b = np.zeros((n, g.S, 4 * g.W), np.uint8)
    b[:, :, :g.R] = rng.integers(0, 256, (n, g.S, g.R), dtype=np.uint8) * rng.integers(0, 2, (n, g.S, g.R), dtype=np.uint8)
    return b.reshape(n, -1).view("<u4").astype(np.uint32)


for n in [int(v) for v in a.rows.split(",")]:
    h = vl.Handle(0, scan_line=16, with_mapping=0)
    h.place_enable(capacity=n)
    rows, tags = random_rows(n), np.arange(n, dtype=np.int32)
    query = rows[n // 3].reshape(g.S, g.W).copy()
    query = np.roll(query, 11, axis=0).reshape(-1)   # row n/3 turned by 11 sectors
    h.place_load(rows, tags)
    h.place_time_query(query, a.warm, k=a.k)
    ms = h.place_time_query(query, a.repeats, k=a.k)
    wall = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        got = h.place_query_descriptor(query, k=a.k)
        wall.append(1e3 * (time.perf_counter() - t0))
    # the bounds: every row read once from HBM; one 4-byte LDS read per lane per row word, a ds_read_b32 wave instruction taking 2 LDS cycles
    hbm_ms = 1e3 * n * g.words * 4 / (a.hbm_tbs * 1e12)
    lds_ms = 1e3 * (n / a.cus) * g.words * 2 / (a.ghz * 1e9)
    line = "rows %7d: device median %.4f ms (min %.4f, max %.4f, %d launches) | call wall median %.4f ms | bounds: HBM %.4f ms, LDS %.4f ms" % (
        n, float(np.median(ms)), float(ms.min()), float(ms.max()), a.repeats, float(np.median(wall)), hbm_ms, lds_ms)
    if n <= a.model_rows:
        t0 = time.perf_counter()
        want = model.records(model.match_all(query, rows, g), tags, n, k=a.k)
        line += " | NumPy model %.1f ms" % (1e3 * (time.perf_counter() - t0))
        assert got.tobytes() == want.tobytes(), (got, want)
        line += " (records equal)"
    print(line, flush=True)
    assert (got[0]["row"], got[0]["shift"], got[0]["dist"]) == (n // 3, 11, 0), got[0]
    h.close()
