"""GPU test of the CLI's -sp N FILE (main.cpp): after optimisation, one line
per (recognized string, sample) -- string, sample index (0 first), log weight of
the path, that weight over q, the path's Fsa parameter indices -- against the
Python learner taking the same steps and sampling with the same seed; a run
with the seed given again writes the same file.  Needs a gfx950 device."""
import os
import subprocess

import numpy as np
import pytest

from conftest import DATA, ROOT

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "w-fsa_amd", "wfsa_amd", "wfsa")
WFSA, CORPUS = os.path.join(DATA, "test3.wfsa"), os.path.join(DATA, "test.corpus")
RUN = [CLI, "-a", WFSA, "-c", CORPUS, "-opt", "QuasiNewton", "-e", "3", "-i", "1", "-s"]


@pytest.mark.parametrize("flag", ["-sp", "--sample-paths"])
def test_sample_paths_file_matches_the_python_learner(flag, tmp_path):
    import wfsa_amd as W
    out, again, other = str(tmp_path / "s.tsv"), str(tmp_path / "again.tsv"), str(tmp_path / "other.tsv")
    r = subprocess.run(RUN + [flag, "6", out, "--sample-seed", "12345678901234"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = open(out, encoding="latin-1").read().split("\n")
    assert lines[-1] == ""
    rows = [l.split("\t") for l in lines[:-1]]
    assert all(len(row) == 5 for row in rows)

    corpus = W.Corpus.read_file(CORPUS)
    lrn = W.QuasiNewtonLearner(0)
    lrn.BuildFrom(W.Fsa.read_file(WFSA), corpus)
    lrn.Finalize()
    lrn.Init(1)
    for _ in range(3):   # the CLI's epoch loop: eta 1, tol 1e-6
        _, halt = lrn.OptimizationStep(1.0, 1e-6)
        if halt:
            break
    srow, logw, prow, pidx, logq = lrn.SamplePaths(6, seed=12345678901234)
    strings, _ = corpus.strings()
    _, rec = lrn.path_counts()
    want = [s for s, k in zip(strings, rec) if k]
    assert len(want) == 4   # test3 recognizes 4 of its 7 strings
    assert list(np.diff(srow)) == [6, 6, 6, 6]
    assert [(row[0], int(row[1])) for row in rows] == [(want[s], t) for s in range(4) for t in range(6)]
    for t, row in enumerate(rows):
        s = t // 6
        assert row[4].split() == [str(j) for j in pidx[prow[t]:prow[t + 1]]]
        got, rel = float(row[2]), float(row[3])
        assert abs(got - logw[t]) <= 1e-12 * abs(logw[t]), (got, logw[t])
        ratio = np.exp(logw[t] - logq[s])
        assert abs(rel - ratio) <= 1e-12 * ratio, (rel, ratio)
        assert rel <= 1.0 + 1e-12

    # the seed given again: the same file; the default seed (0): other draws for the ambiguous strings
    r = subprocess.run(RUN + [flag, "6", again, "--sample-seed", "12345678901234"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(out, "rb").read() == open(again, "rb").read()
    r = subprocess.run(RUN + [flag, "6", other], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    srow0, logw0, prow0, pidx0, _ = lrn.SamplePaths(6)
    assert [row.split("\t")[4].split() for row in open(other, encoding="latin-1").read().split("\n")[:-1]] == \
        [[str(j) for j in pidx0[prow0[t]:prow0[t + 1]]] for t in range(24)]


def test_usage_names_the_option():
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--sample-paths N FILE" in r.stderr and "--sample-seed S" in r.stderr
