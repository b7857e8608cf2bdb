"""GPU test of the CLI's -pc FILE (main.cpp): after optimisation, one line per
recognized string in corpus order -- string, log q, entropy, then id:count per
Fsa parameter in ascending id, counts at %.17g -- against the Python learner
taking the same steps; refused in matrix-file mode (no -a / -c).  Needs a
gfx950 device."""
import os
import subprocess

import numpy as np
import pytest

from conftest import DATA, ROOT

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "w-fsa_amd", "wfsa_amd", "wfsa")
WFSA, CORPUS = os.path.join(DATA, "talk.wfsa"), os.path.join(DATA, "talk.corpus")
RUN = [CLI, "-a", WFSA, "-c", CORPUS, "-opt", "QuasiNewton", "-e", "3", "-i", "1", "-s"]


@pytest.mark.parametrize("flag", ["-pc", "--posterior-counts"])
def test_posterior_counts_file_matches_the_python_learner(flag, tmp_path):
    import wfsa_amd as W
    out = str(tmp_path / "pc.tsv")
    r = subprocess.run(RUN + [flag, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = open(out, encoding="latin-1").read().split("\n")
    assert lines[-1] == ""
    rows = [l.split("\t") for l in lines[:-1]]

    corpus = W.Corpus.read_file(CORPUS)
    lrn = W.QuasiNewtonLearner(0)
    lrn.BuildFrom(W.Fsa.read_file(WFSA), corpus)
    lrn.Finalize()
    lrn.Init(1)
    for _ in range(3):   # the CLI's epoch loop: eta 1, tol 1e-6
        _, halt = lrn.OptimizationStep(1.0, 1e-6)
        if halt:
            break
    crow, cidx, cval, logq, entropy = lrn.PosteriorCounts()
    strings, _ = corpus.strings()
    _, rec = lrn.path_counts()
    want = [s for s, k in zip(strings, rec) if k]
    assert len(want) == 3 and len(crow) == 4   # talk recognizes 3 of its 5 strings
    assert [row[0] for row in rows] == want
    for s, row in enumerate(rows):
        # %.17g round-trips a double
        assert float(row[1]) == logq[s] and float(row[2]) == entropy[s]
        pairs = [p.split(":") for p in row[3:]]
        assert [int(p[0]) for p in pairs] == list(cidx[crow[s]:crow[s + 1]]) and len(pairs) > 0
        assert [float(p[1]) for p in pairs] == list(cval[crow[s]:crow[s + 1]])
        assert np.isfinite(logq[s]) and entropy[s] >= 0.0


def test_refused_without_an_automaton(tmp_path):
    prefix = str(tmp_path / "m")
    r = subprocess.run([CLI, "-a", WFSA, "-c", CORPUS, "-opt", "QuasiNewton", "-e", "0", "-s", "-m", ">" + prefix],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = str(tmp_path / "pc.tsv")
    r = subprocess.run([CLI, "-m", "<" + prefix, "-opt", "QuasiNewton", "-e", "1", "-i", "1", "-s", "-pc", out],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "-pc needs an automaton and a corpus" in r.stderr
    assert not os.path.exists(out)


def test_usage_names_the_option():
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--posterior-counts FILE" in r.stderr
