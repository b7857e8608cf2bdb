"""GPU test of the CLI's -kbp K FILE (main.cpp): after optimisation, one line
per (recognized string, rank) -- string, rank (1 = best), log weight of the
path, that weight over q, the path's Fsa parameter indices -- against the
Python learner taking the same steps; -bp beside it is unchanged.  Needs a
gfx950 device."""
import os
import subprocess

import numpy as np
import pytest

from conftest import DATA, ROOT

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "w-fsa_amd", "wfsa_amd", "wfsa")
WFSA, CORPUS = os.path.join(DATA, "test3.wfsa"), os.path.join(DATA, "test.corpus")
RUN = [CLI, "-a", WFSA, "-c", CORPUS, "-opt", "QuasiNewton", "-e", "3", "-i", "1", "-s"]


@pytest.mark.parametrize("flag", ["-kbp", "--k-best-paths"])
def test_kbest_paths_file_matches_the_python_learner(flag, tmp_path):
    import wfsa_amd as W
    out, best, alone = str(tmp_path / "kbest.tsv"), str(tmp_path / "best.tsv"), str(tmp_path / "alone.tsv")
    r = subprocess.run(RUN + [flag, "3", out, "-bp", best], capture_output=True, text=True, timeout=120)
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
    srow, logw, prow, pidx = lrn.KBestPaths(3)
    _, _, logq = lrn.objective_grad(want_logq=True)
    strings, _ = corpus.strings()
    _, rec = lrn.path_counts()
    want = [s for s, k in zip(strings, rec) if k]
    assert len(want) == 4   # test3 recognizes 4 of its 7 strings, with 1, 2, 3 and 1 paths
    assert list(np.diff(srow)) == [1, 2, 3, 1]
    assert [(row[0], int(row[1])) for row in rows] == [(want[s], t - srow[s] + 1) for s in range(4)
                                                       for t in range(srow[s], srow[s + 1])]
    line = 0
    for s in range(4):
        for t in range(srow[s], srow[s + 1]):
            row = rows[line]
            line += 1
            assert row[4].split() == [str(j) for j in pidx[prow[t]:prow[t + 1]]]
            got, rel = float(row[2]), float(row[3])
            assert abs(got - logw[t]) <= 1e-12 * abs(logw[t]), (got, logw[t])
            ratio = np.exp(logw[t] - logq[s])
            assert abs(rel - ratio) <= 1e-12 * ratio, (rel, ratio)
            assert rel <= 1.0 + 1e-12

    # the -bp file of the same run is the one written without -kbp
    r = subprocess.run(RUN + ["-bp", alone], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(best, "rb").read() == open(alone, "rb").read()
    assert len(open(alone, "rb").read().split(b"\n")) == 5


def test_usage_names_the_option():
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--k-best-paths K FILE" in r.stderr
