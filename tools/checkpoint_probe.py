#!/usr/bin/env python3
"""Checkpoint and restore, measured (profiles/r07_checkpoint.txt): the 64 x 2048 bench map after N sweeps — checkpoint size, wall time of
vloam_checkpoint_size / _save / _load, and the map kernels' own times (VLOAM_CKPT_TIMES=1 makes the library print them: count + scan and
pack for a save, unpack for a load), per table size.  Usage: python tools/checkpoint_probe.py [--sweeps 200] [--log2 19 22]"""
import argparse
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["VLOAM_CKPT_TIMES"] = "1"
_seq = None


def _sweep(k):
    global _seq
    import conftest
    synth = conftest.load_synth()
    if _seq is None:
        _seq = synth.SynthSequence(n_rings=64, n_azimuth=2048, n_sweeps=int(os.environ["CKPT_PROBE_T"]) + 1)
    return _seq.sweep(k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=200)
    ap.add_argument("--log2", type=int, nargs="+", default=[19, 22])
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    os.environ["CKPT_PROBE_T"] = str(a.sweeps)
    with ProcessPoolExecutor(16) as ex:   # before HIP exists in this process
        clouds = list(ex.map(_sweep, range(a.sweeps), chunksize=4))
    import conftest
    vl = conftest.load_pkg()
    n_pts = max(c.shape[0] for c in clouds)
    for lg in a.log2:
        h = vl.Handle(0, with_mapping=1, map_capacity_log2=lg, max_points=n_pts, max_frames=a.sweeps + 8)
        for c in clouds:
            h.process_scan(c)
        h.sync()
        mh = h.map_health()
        print("table 2^%d: %d sweeps, keys %s, purged %s, block keys %s, map points %d" % (lg, a.sweeps, mh["keys"], mh["purged"], mh["block_keys"], h.get_map().shape[0]), flush=True)
        for r in range(a.repeats):
            t0 = time.perf_counter()
            data = h.checkpoint()   # vloam_checkpoint_size + vloam_checkpoint_save
            t1 = time.perf_counter()
            sys.stderr.flush()
            print("  save %d: %.2f ms wall (size + save), %d bytes" % (r, 1e3 * (t1 - t0), len(data)), flush=True)
        h.close()
        for r in range(a.repeats):
            c = vl.Handle(0, with_mapping=1, map_capacity_log2=lg, max_points=n_pts, max_frames=a.sweeps + 8)
            t0 = time.perf_counter()
            c.restore(data)
            t1 = time.perf_counter()
            sys.stderr.flush()
            print("  load %d: %.2f ms wall" % (r, 1e3 * (t1 - t0)), flush=True)
            c.close()


if __name__ == "__main__":
    main()
