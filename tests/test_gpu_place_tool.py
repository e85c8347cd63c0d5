"""GPU: tools/run_sequence.py --place-db / --relocalize-global — a synthetic drive saved with its place database, then sweep j of the same drive
localised against the loaded map with no start pose: the place match names row j at distance 0 and shift 0, and from there the run is the
existing --relocalize path, byte for byte what --start-pose with row j's saved pose gives."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import place_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_global_relocalisation_from_the_place_database(tmp_path, synth):
    n = 4
    drive = ["--synthetic", str(n), "--azimuth", "256", "--mapping-skip-frame", "1"]
    tool = [sys.executable, os.path.join(ROOT, "tools", "run_sequence.py")]
    run = lambda extra: subprocess.run(tool + drive + extra, capture_output=True, text=True, timeout=600)
    r = run(["--out", str(tmp_path / "a"), "--place-db", "--save-map", str(tmp_path / "map")])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "wrote %d place rows" % n in r.stdout, r.stdout
    db = np.load(tmp_path / "map" / "place_db.npz")
    assert db["desc"].shape == (n, 300) and db["tags"].tolist() == list(range(n)) and db["poses"].shape == (n, 7)
    g = model.Geometry(int(db["n_ring"]), int(db["n_sector"]), db["min_range"].item(), db["max_range"].item(), db["z_min"].item(), db["z_step"].item())
    assert (g.R, g.S, float(g.max_range), float(g.z_min)) == (20, 60, 80.0, -3.0)
    # the model on the CPU: the sweeps whose own row is the only one at distance 0; the last of them is j
    alone = [k for k in range(n) if np.flatnonzero(model.match_all(db["desc"][k], db["desc"], g)[0] == 0).tolist() == [k]]
    assert alone, "every sweep of the drive has a twin"
    j = alone[-1]
    seq = synth.SynthSequence(n_rings=64, n_azimuth=256, n_sweeps=max(n, 2) + 1)
    desc, _ = model.describe(seq.sweep(j), g)
    assert desc.tobytes() == db["desc"][j].tobytes()   # the saved row is the model's descriptor of that sweep
    want = model.query(desc, db["desc"], db["tags"], g)[0]
    assert (want["row"], want["tag"], want["shift"], want["dist"]) == (j, j, 0, 0)
    grid = "1 0.5 5 2.5 2"
    load = ["--load-map", str(tmp_path / "map"), "--localize-only", "--first-sweep", str(j)]
    ra = run(["--out", str(tmp_path / "g"), "--metrics", str(tmp_path / "g.jsonl"), "--relocalize-global", grid] + load)
    assert ra.returncode == 0, ra.stdout + ra.stderr
    assert "place match: row %d, tag %d, shift 0, dist 0\n" % (j, j) in ra.stdout, ra.stdout
    pose = " ".join("%.17g" % v for v in db["poses"][j])
    rb = run(["--out", str(tmp_path / "s"), "--metrics", str(tmp_path / "s.jsonl"), "--start-pose", pose, "--relocalize", grid] + load)
    assert rb.returncode == 0, rb.stdout + rb.stderr
    # the same existing code from the same centre: output byte-equal, plus the one line naming the match
    assert "relocalised sweep 0: candidate" in rb.stdout and "localised %d sweeps" % (n - j) in rb.stdout, rb.stdout
    lines_a = [ln for ln in ra.stdout.replace(str(tmp_path / "g"), "OUT").splitlines() if not ln.startswith("place match:")]
    assert lines_a == rb.stdout.replace(str(tmp_path / "s"), "OUT").splitlines()
    assert len(ra.stdout.splitlines()) == len(lines_a) + 1
    for name in ("LOC0.txt",):
        assert open(tmp_path / "g" / name, "rb").read() == open(tmp_path / "s" / name, "rb").read()
    assert open(tmp_path / "g.jsonl", "rb").read() == open(tmp_path / "s.jsonl", "rb").read()
    # without a saved database the option says what to do
    os.remove(tmp_path / "map" / "place_db.npz")
    r = run(["--out", str(tmp_path / "x"), "--relocalize-global", grid] + load)
    assert r.returncode != 0 and "--place-db --save-map" in r.stderr, r.stderr
    assert re.search(r"place_db\.npz", r.stderr)
