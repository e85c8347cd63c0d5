"""-m gpu: the two per-sweep row products (sweep log, pose information) read WITHOUT vloam_sync once the event ring behind the row writes has wrapped.

Every stage's row write of sweep k is bound to an event in slot k % 16 (2 * kBufferSets) of a ring; a getter waits for the events of the LAST row
asked for, and only where the slot still carries that sweep's number.  20 sweeps bind slots 0 - 3 twice: a row whose slot a later sweep has taken
over is read without a wait (its writes finished long before the later sweep could be enqueued), a row still in flight is waited for.  The
reference is a handle that processed the same sweeps, synchronised, and read both products in full; integer fields and `frame` compare exactly,
floating fields with the bounds of tests/test_gpu_sweep_log.py and tests/test_gpu_pose_info.py.  Row 0 of the selected session sits at an arena
offset for the sweep log and at sel * max_frames rows for pose information: the batched case reads session 1."""
import numpy as np
import pytest

from test_gpu_batch import sequences
from test_gpu_pose_info import rows_close
from test_gpu_sweep_log import assert_costs, assert_ints

pytestmark = pytest.mark.gpu

SHAPE = (16, 256)
N = 20   # > 2 * kBufferSets = 16 event slots per stage
# (sweeps handed over, [(first, count), ...]): the reads of a handle that never synchronises
READS = [(12, [(0, 4)]),
         (18, [(1, 2), (0, 2), (16, 2)]),   # rows 0 and 1: their slots now carry sweeps 16 and 17; rows 16 and 17 are in flight
         (20, [(0, 20)])]

_ref = {}


def reference(vl, synth):
    """Session 1's sequence of the batched case, alone, synchronised, both products in full: computed once."""
    if not _ref:
        seqs = sequences(synth, 2, N, shape=SHAPE)
        h = vl.Handle(0, scan_line=SHAPE[0], with_mapping=1, sweep_log=1)
        h.enable_pose_info()
        for c in seqs[1]:
            h.process_scan(c)
        h.sync()
        log, info = h.sweep_log().copy(), h.pose_info().copy()
        h.close()
        assert log.shape == (N,) and info.shape == (N,) and log["frame"].tolist() == list(range(N)) and info["frame"].tolist() == list(range(N))
        _ref.update(seqs=seqs, log=log, info=info)
    return _ref


def read_behind_the_pipeline(vl, h, feed, ref, exact_costs):
    fed = 0
    for upto, reads in READS:
        while fed < upto:
            feed(fed)
            fed += 1
        assert h.frame_count() == upto
        for first, count in reads:
            what = "rows %d .. %d behind %d sweeps" % (first, first + count - 1, upto)
            log, info = h.sweep_log(first, count), h.pose_info(first, count)
            assert log["frame"].tolist() == list(range(first, first + count)), what
            assert info["frame"].tolist() == list(range(first, first + count)), what
            assert_ints(log, ref["log"][first:first + count], what)
            if exact_costs:
                assert_costs(log, ref["log"][first:first + count], what)
            rows_close(vl, info, ref["info"][first:first + count])


def test_single_sequence(vl, synth):
    ref = reference(vl, synth)
    h = vl.Handle(0, scan_line=SHAPE[0], with_mapping=1, sweep_log=1)
    h.enable_pose_info()
    read_behind_the_pipeline(vl, h, lambda k: h.process_scan(ref["seqs"][1][k]), ref, exact_costs=True)
    h.close()


def test_session_1_of_a_batch(vl, synth):
    ref = reference(vl, synth)
    seqs = ref["seqs"]
    h = vl.Handle(0, n_sessions=2, scan_line=SHAPE[0], with_mapping=1, sweep_log=1)
    h.enable_pose_info()
    h.select(1)
    # (a batch's solves add in another order: the costs of the log are left to tests/test_gpu_sweep_log.py, as in its own batch test)
    read_behind_the_pipeline(vl, h, lambda k: h.batch_process_scan([seqs[0][k], seqs[1][k]]), ref, exact_costs=False)
    other = h.select(0).sweep_log()
    assert not np.array_equal(other["n_cloud"], ref["log"]["n_cloud"]), "the sessions are different sequences"
    h.close()
