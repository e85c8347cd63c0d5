"""CPU: the oracle's depth-enhanced visual odometry (oracle/orc_vo.cpp) against the REFERENCE'S OWN point_cloud_util.cpp and
visual_odometry.cpp::solveNlsAll, compiled unmodified (oracle/_ref/libref_vo.so through oracle/ref.py; stand-in headers in
oracle/ref_shim/; harness oracle/ref_vo_harness.cpp).

Bit for bit (f32 pipelines with a fixed evaluation order): point_cloud_2d; the four bucket matrices; point_cloud_2d_dnsp (the non-empty
buckets in reverse scan order); queryDepth for every listed pixel; per match the kind (CostFunctor32 / CostFunctor22 / skipped), depth0
and the functor's observations in AddResidualBlock order.  Exact: both counters, the integer pixel pairs against the oracle's front half
(orc.orb_matches / orc.flow_matches: float -> int truncation, status == 1), the parameters ceres::Solve starts from.  The solve:
POSE_TOL of tests/test_ref_laser_odometry.py — the minimizer behind both sides is the same code (oracle/ref_bridge.cpp).

queryDepth sorts its neighbours with std::sort, so neighbours at equal distance have no defined order.  The oracle's canonical order is
the scan order (std::stable_sort).  The reference's build here is libstdc++, whose std::sort is an insertion sort — which keeps the scan
order — up to 16 elements and an introsort above, so with 17 to 25 neighbours its order is open.  A pixel whose third and fourth
smallest distances are equal (the harness flags it) is therefore compared only on what no order changes: whether the answer is -1.  The
share of such pixels is printed and must stay within 1 % in every scenario.

One case of the plan cannot exist: depth0 == 0 exactly.  queryDepth returns -1 or a quotient whose numerator is a sum of products of
bucket depths (each > 0.1: only such points are folded, and the incremental mean stays between its inputs) and distances of which at most
one can be zero (two buckets never hold the same mean), over a positive denominator — so it is positive.  The `depth0 > 0` branch is
exercised from -1 and from the smallest depths the projection lets through (0.1f's upper neighbour).

Also here: the committed recordings tests/golden/ref_vo_*.npz are what the reference binary gives now (tests/test_gpu_ref_pinned_vo.py
compares the device with them on a machine that has neither the reference nor the binary).

Skips: only when neither the reference checkout nor a built oracle/_ref/libref_vo.so exists.
"""
import os

import numpy as np
import pytest

import ref_vo_cases as cases

import ref

pytestmark = pytest.mark.skipif(not ref.vo_available(), reason=ref.SKIP_REASON)

POSE_TOL = 1e-8     # tests/test_ref_laser_odometry.py
HERE = os.path.dirname(os.path.abspath(__file__))
STEMS = ["ref_vo_64x256_3frames", "ref_vo_64x256_perturbed", "ref_vo_edges", "ref_vo_match_loop"]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def scenarios():
    return cases.scenarios()


@pytest.fixture(scope="module")
def recordings(scenarios):
    """Every scenario through the reference binary, once for the whole module."""
    return {stem: cases.record(ref, sc) for stem, sc in scenarios.items()}


def test_the_scenarios_are_the_committed_ones(scenarios):
    assert sorted(scenarios) == sorted(STEMS)


def check_queries(o, d, k, what):
    xy, want, tie = d["f%d_qxy" % k], d["f%d_qdepth" % k], d["f%d_qtie" % k].astype(bool)
    got = np.array([o.query_depth(0, x, y) for x, y in xy], dtype=np.float32)
    assert np.array_equal(got == -1.0, want == -1.0), "%s: which pixels have no depth" % what
    assert same_bits(got[~tie], want[~tie]), "%s: queryDepth" % what
    return int(np.count_nonzero(want == -1.0)), int(np.count_nonzero(want > 0))


def front_half(orc, run, flow):
    """The integer pixel pairs as the ORACLE'S front half derives them from what the front-end left."""
    if flow:
        return orc.flow_matches(run["kp_prev"], run["kp_curr"], run["status"])
    return run["kp_prev"][run["query_idx"]].astype(np.int32), run["kp_curr"][run["train_idx"]].astype(np.int32)   # orc.orb_matches' last line


@pytest.mark.parametrize("stem", STEMS)
def test_oracle_against_the_reference_binary(orc, scenarios, recordings, stem):
    sc, d = scenarios[stem], recordings[stem]
    ties, nq = cases.tie_share(d)
    print("%s: %d of %d queried pixels tie on the third / fourth neighbour (%.3f %%)" % (stem, ties, nq, 100.0 * ties / max(nq, 1)))
    assert ties <= 0.01 * nq, "the generator refuses a fixture with more than 1 % ties: choose other seeds"
    seen = dict(minus1=0, positive=0, k32=0, k22=0, skipped=0, nomatch=0)
    for si, s in enumerate(sc["sessions"]):
        o = orc.VOOracle(*sc["calib"], remove_outlier=s["remove_outlier"])
        for k, c in enumerate(sc["frames"]):
            w = "%s session %d frame %d" % (stem, si, k)
            o.reset()
            o.process_point_cloud(c)
            if si == 0:
                assert d["f%d_p2d" % k].shape[0] > 1000
                assert same_bits(o.points2d(0), d["f%d_p2d" % k]), "%s: point_cloud_2d" % w
                ob, rb = o.buckets(0), cases.dense(d, k)
                assert np.array_equal(ob[3], rb[3]), "%s: bucket_count" % w
                for a, name in enumerate(("bucket_x", "bucket_y", "bucket_depth")):
                    assert same_bits(ob[a], rb[a]), "%s: %s" % (w, name)
                idx = np.nonzero(ob[3])[0]
                assert same_bits(np.stack([ob[0][idx], ob[1][idx], ob[2][idx]], axis=1)[::-1], d["f%d_dnsp" % k]), "%s: point_cloud_2d_dnsp" % w
                if k > 0:   # the previous frame's map is still the one recorded a frame ago (count % 2 ping-pong; frame 2 overwrites frame 0's)
                    pb, rp = o.buckets(1), cases.dense(d, k - 1)
                    assert np.array_equal(pb[3], rp[3]) and all(same_bits(pb[a], rp[a]) for a in range(3)), "%s: the previous frame's map" % w
                if "f%d_qxy" % k in d:
                    m1, pos = check_queries(o, d, k, w)
                    seen["minus1"] += m1
                    seen["positive"] += pos
            if k not in s["runs"]:
                continue
            run, pre = s["runs"][k], "s%d_r%d_" % (si, k)
            rows, x_in, x_out, cnt = d[pre + "rows"], d[pre + "x_in"], d[pre + "x_out"], d[pre + "counters"]
            is_match = rows[:, 0] != -1
            pu, cu = front_half(orc, run, s["optical_flow_match"])
            assert np.array_equal(pu, rows[is_match, 7:9]) and np.array_equal(cu, rows[is_match, 9:11]), "%s: integer pixel pairs" % w
            if s["optical_flow_match"]:
                assert np.array_equal(is_match, run["status"] == 1), "%s: optical_flow_status == 1" % w
            if s["reset_to_identity"]:
                assert not x_in.any(), "%s: reset_VO_to_identity" % w
                r = o.solve(pu, cu, None, None)
            else:
                q, t = run["prior_q"], run["prior_t"]
                th = 2 * np.arctan2(np.linalg.norm(q[:3]), q[3])
                aa = q[:3] / np.linalg.norm(q[:3]) * th if th > 0 else np.zeros(3)
                assert np.max(np.abs(x_in[:3] - aa)) < 1e-12 and np.max(np.abs(x_in[3:] - t)) < 1e-15, "%s: the prior through tf2" % w
                r = o.solve(pu, cu, x_in[:3], x_in[3:])
            md = r["match_debug"]
            assert np.array_equal(md[:, 0], rows[is_match, 0]), "%s: kinds" % w
            assert same_bits(md[:, 1], rows[is_match, 1]), "%s: depth0" % w
            assert np.array_equal(md[:, 2:], rows[is_match, 2:7]), "%s: observations" % w
            assert (r["counter32"], r["counter22"]) == tuple(int(v) for v in cnt), "%s: counters" % w
            assert cnt[0] == np.count_nonzero(rows[:, 0] == 32) and cnt[1] == np.count_nonzero(rows[:, 0] == 22)
            assert np.linalg.norm(r["angles"] - x_out[:3]) < POSE_TOL and np.linalg.norm(r["t"] - x_out[3:]) < POSE_TOL, "%s: the solve" % w
            if cnt.sum() == 0:
                assert np.array_equal(x_out, x_in) and np.array_equal(r["angles"], x_in[:3]) and np.array_equal(r["t"], x_in[3:]), "%s: nothing to solve" % w
            for key, kind in (("k32", 32), ("k22", 22), ("skipped", 0), ("nomatch", -1)):
                seen[key] += int(np.count_nonzero(rows[:, 0] == kind))
            seen["minus1"] += int(np.count_nonzero(rows[:, 1] == -1.0))
    print(stem, seen)
    assert seen["k32"] > 30 and seen["k22"] > 30 and seen["minus1"] > 30


def test_the_edge_scenario_hits_its_edges(recordings):
    """On the REFERENCE'S output: the points and buckets the scenario was built for are there."""
    d = recordings["ref_vo_edges"]
    tenth = np.float32(0.1)
    for k in range(2):
        p, (bx, by, bd, bc) = d["f%d_p2d" % k], cases.dense(d, k)
        u, v, z = p[:, 0], p[:, 1], p[:, 2]
        assert z.min() == np.nextafter(tenth, np.float32(1)), "depth 0.1f and below are screened out (> 0.1), its upper neighbour is kept"
        assert np.count_nonzero(z < 1.0) == 1
        for lo, hi, col in ((-5, 0, u), (-5, 0, v), (1240, 1245, u), (1245, 1250, u), (370, 375, v), (375, 380, v)):
            assert np.count_nonzero((col > lo) & (col < hi)) >= 2, (lo, hi)
        # truncation toward zero: a point with u in (-5, 0) lands in bucket column 0 (floor would drop it); one past the last bucket is dropped
        for i in np.nonzero((u > -5) & (u < 0) & (v > 0) & (v < 370))[0]:
            assert bc[0 * cases.NBY + int(v[i] / 5)] >= 1
        both = np.nonzero((u > -5) & (u < 0) & (v > -5) & (v < 0))[0]
        assert both.size == 1 and bc[0] >= 1
        inside = (u > -5) & (u < 1245) & (v > -5) & (v < 375)
        assert bc.sum() == np.count_nonzero(inside), "every point within (-5, 1245) x (-5, 375) is folded, no other"
        assert bc[248 * cases.NBY + 40] >= 1 and bc[140 * cases.NBY + 74] >= 1, "the last bucket column and row"
        for (cx, cy), cnt in cases.CLUSTERS.items():
            assert bc[cx * cases.NBY + cy] == cnt
        q = d["f%d_qdepth" % k]
        assert np.count_nonzero(q == -1.0) > 1000 and np.count_nonzero(q > 0) > 1000, "pixels with fewer than ten filled neighbours, and with enough"
        assert np.all((q == -1.0) | (q > 0))


def test_the_match_loop_scenario_hits_its_edges(scenarios, recordings):
    sc, d = scenarios["ref_vo_match_loop"], recordings["ref_vo_match_loop"]
    rows = d["s0_r1_rows"]
    ga, _ = cases.gate_pairs()
    assert np.array_equal(rows[-12:, 7:9], np.floor(ga)), "a float keypoint becomes an int by truncation"
    assert np.all(rows[-12:-8, 0] != 0), "squared distance == remove_VO_outlier^2: kept, the gate is >"
    assert np.all(rows[-8:-4, 0] == 0) and np.all(rows[-4:, 0] != 0), "one pixel farther: skipped; one nearer: kept"
    far = d["s1_r1_rows"]
    dist2 = (far[:, 7] - far[:, 9]) ** 2 + (far[:, 8] - far[:, 10]) ** 2
    assert np.count_nonzero(dist2 > 100 ** 2) > 100 and np.all(far[:, 0] != 0), "remove_VO_outlier = 0 turns the gate off"
    flow, status = d["s2_r1_rows"], sc["sessions"][2]["runs"][1]["status"]
    assert np.array_equal(flow[:, 0] == -1, status != 1) and np.count_nonzero(status == 0) > 20 and np.count_nonzero(status == 2) > 20
    assert not d["s3_r1_x_in"].any(), "the identity prior: angle 0 times the arbitrary axis"
    assert np.linalg.norm(d["s4_r1_x_in"][:3]) > 0.02 and np.linalg.norm(d["s4_r1_x_out"] - d["s4_r1_x_in"]) > 1e-3
    assert np.all(d["s5_r1_rows"][:, 0] == 0) and not d["s5_r1_counters"].any(), "no usable match"
    assert np.array_equal(d["s5_r1_x_out"], d["s5_r1_x_in"]) and d["s5_r1_x_in"][5] == 0.8


@pytest.mark.parametrize("stem", STEMS)
def test_the_committed_recording_is_what_the_reference_binary_gives(recordings, stem):
    d, z = recordings[stem], np.load(os.path.join(HERE, "golden", stem + ".npz"))
    assert sorted(d) == sorted(z.files)
    for key in sorted(d):
        a, b = np.asarray(d[key]), z[key]
        assert a.shape == b.shape and a.dtype == b.dtype, key
        if key.endswith("_x_out"):
            assert np.max(np.abs(a - b), initial=0) < POSE_TOL, key
        else:
            assert np.array_equal(a, b, equal_nan=True), key
