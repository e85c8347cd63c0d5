"""CPU: the stream plan of a handle (csrc/stream_plan.h) — which priority level, and so which of the runtime's hardware-queue pools, each stream
of a handle is created in, from GPU_MAX_HW_QUEUES and the handle kind.  The header is compiled on its own with g++ next to a model of the
runtime's placement rule (tests/cpp/stream_plan.cpp: a queue per stream while the pool has room, then the least-used queue of the pool), which
predicts the queue of every stream for every budget from 1 to 32 and a host that holds 1 - 6 normal-priority queues of its own before the
handle is created.  Limits: the model is the rule measured once (profiles/r07_hw_queue_map.txt), so this test checks the plan against that
rule, not the runtime; where streams land on a GPU is read from a kernel trace (tools/queue_map.py), not asserted by any test."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR, LO, MAP, DS, IMG, COPY = range(6)
NORMAL, HIGH, LOW = 0, 1, 2


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stream_plan") / "stream_plan")
    subprocess.run(["g++", "-O1", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "vloam-cmu-16833_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "stream_plan.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    res = []
    for ln in out:
        if ln:
            v = [int(x) for x in ln.split()]
            res.append(dict(budget=v[0], mapping=v[1], image=v[2], host=v[3], pooled=v[4], copy_first=v[5], pool=v[6:12], queue=v[12:18]))
    assert len(res) == 32 * 2 * 2 * 6
    return res


def test_period_bounding_stages_never_share_a_queue(rows):
    """SR, LO and mapping on three different queues: in the pooled plan whatever the host holds, in the flat one while the host keeps within
    the reserve the plan leaves it."""
    for r in rows:
        if not r["pooled"] and r["host"] > 1 + 4:
            continue
        q = [r["queue"][s] for s in (SR, LO, MAP) if r["queue"][s] >= 0]
        assert len(set(q)) == len(q), r


def test_the_voxelgrid_wait_never_sits_in_front_of_another_stage(rows):
    """The scan-feature VoxelGrid waits for the scan registration of its sweep (a live wait): its queue is its own, or the scan registration's
    (where the wait is behind the work it waits for)."""
    for r in rows:
        if not r["mapping"] or (not r["pooled"] and r["host"] > 1 + 4):
            continue
        for s in (LO, MAP, IMG):
            assert r["queue"][s] != r["queue"][DS], r
        if r["budget"] >= 3:
            assert r["queue"][COPY] != r["queue"][DS], r


def test_every_stream_has_a_queue_of_its_own_from_three_queues_on(rows):
    """... while the host's normal-priority streams leave room: in the pooled plan odometry and images share the normal pool with them."""
    for r in rows:
        if r["budget"] >= 3 and (r["host"] <= 1 if r["pooled"] else r["host"] <= 1 + 4):
            q = [x for x in r["queue"] if x >= 0]
            assert len(set(q)) == len(q), r


def test_sixteen_queues_keep_every_stream_at_normal_priority(rows):
    """The budget the package and bench.py ask for (and anything above): the plan of the handles before it, one pool."""
    for r in rows:
        if r["budget"] >= 16:
            assert not r["pooled"] and r["copy_first"] and all(p in (-1, NORMAL) for p in r["pool"]), r


def test_the_default_budget_spreads_the_stages_over_the_three_pools(rows):
    for r in rows:
        if r["budget"] == 4:
            assert r["pooled"], r
            assert (r["pool"][SR], r["pool"][LO]) == (LOW, NORMAL), r
            assert r["pool"][MAP] == (HIGH if r["mapping"] else -1), r
