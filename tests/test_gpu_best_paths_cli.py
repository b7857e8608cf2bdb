"""GPU test of the CLI's -bp FILE (main.cpp): after optimisation, one line per
recognized string -- string, log weight of its most probable path, that
weight over q, the path's Fsa parameter indices -- against the Python learner
taking the same steps.  Needs a gfx950 device."""
import os
import subprocess

import numpy as np
import pytest

from conftest import DATA, ROOT

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "w-fsa_amd", "wfsa_amd", "wfsa")


@pytest.mark.parametrize("flag", ["-bp", "--best-paths"])
def test_best_paths_file_matches_the_python_learner(flag, tmp_path):
    import wfsa_amd as W
    wpath, cpath = os.path.join(DATA, "talk.wfsa"), os.path.join(DATA, "talk.corpus")
    out = str(tmp_path / "best.tsv")
    r = subprocess.run([CLI, "-a", wpath, "-c", cpath, "-opt", "QuasiNewton", "-e", "3", "-i", "1", "-s", flag, out],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = open(out, encoding="latin-1").read().split("\n")
    assert lines[-1] == ""
    rows = [l.split("\t") for l in lines[:-1]]
    assert all(len(row) == 4 for row in rows)

    corpus = W.Corpus.read_file(cpath)
    lrn = W.QuasiNewtonLearner(0)
    lrn.BuildFrom(W.Fsa.read_file(wpath), corpus)
    lrn.Finalize()
    lrn.Init(1)
    for _ in range(3):   # the CLI's epoch loop: eta 1, tol 1e-6
        _, halt = lrn.OptimizationStep(1.0, 1e-6)
        if halt:
            break
    logw, prow, pidx = lrn.BestPaths()
    _, _, logq = lrn.objective_grad(want_logq=True)
    strings, _ = corpus.strings()
    _, rec = lrn.path_counts()
    want = [s for s, k in zip(strings, rec) if k]
    assert len(want) == 3   # talk recognizes 3 of its 5 strings
    assert [row[0] for row in rows] == want
    for s, row in enumerate(rows):
        assert row[3].split() == [str(j) for j in pidx[prow[s]:prow[s + 1]]]
        got, rel = float(row[1]), float(row[2])
        assert abs(got - logw[s]) <= 1e-12 * abs(logw[s]), (got, logw[s])
        ratio = np.exp(logw[s] - logq[s])
        assert abs(rel - ratio) <= 1e-12 * ratio, (rel, ratio)
        assert rel <= 1.0 + 1e-12


def test_usage_names_the_option():
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--best-paths FILE" in r.stderr
