"""GPU test of the CLI's -bm FILE and -md FILE (main.cpp): after optimisation,
one line per recognized string in corpus order.  -bm: string, log q, then per
byte its boundary probability and the comma-separated state-name:mass list in
ascending state id; -md: string, score, log weight, the MEA path's Fsa parameter
ids.  Both against the Python learner taking the same steps; refused in
matrix-file mode (no -a / -c).  Needs a gfx950 device."""
import os
import subprocess

import numpy as np
import pytest

from conftest import DATA, ROOT

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "w-fsa_amd", "wfsa_amd", "wfsa")
WFSA, CORPUS = os.path.join(DATA, "test3.wfsa"), os.path.join(DATA, "test.corpus")
RUN = [CLI, "-a", WFSA, "-c", CORPUS, "-opt", "QuasiNewton", "-e", "3", "-i", "1", "-s"]


def test_files_match_the_python_learner(tmp_path):
    import wfsa_amd as W
    bm, md = str(tmp_path / "bm.tsv"), str(tmp_path / "md.tsv")
    r = subprocess.run(RUN + ["-bm", bm, "--mea-decode", md], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]

    corpus = W.Corpus.read_file(CORPUS)
    fsa = W.Fsa.read_file(WFSA)
    lrn = W.QuasiNewtonLearner(0)
    lrn.BuildFrom(fsa, corpus)
    lrn.Finalize()
    lrn.Init(1)
    for _ in range(3):   # the CLI's epoch loop: eta 1, tol 1e-6
        _, halt = lrn.OptimizationStep(1.0, 1e-6)
        if halt:
            break
    mrow, midx, mval, boundary, logq, score, plw, prow, pidx = lrn.ByteMarginals(True)
    names = fsa.state_names()
    assert set(names) == {"^", "$", "X", "Y"}
    strings, _ = corpus.strings()
    _, rec = lrn.path_counts()
    want = [s for s, k in zip(strings, rec) if k]
    assert len(want) > 0 and len(logq) == len(want) and len(boundary) == sum(len(s) for s in want)

    lines = open(bm, encoding="latin-1").read().split("\n")
    assert lines[-1] == ""
    rows = [l.split("\t") for l in lines[:-1]]
    assert [row[0] for row in rows] == want
    b = 0
    for s, row in enumerate(rows):
        assert float(row[1]) == logq[s] and len(row) == 2 + 2 * len(want[s])   # %.17g round-trips a double
        for i in range(len(want[s])):
            assert float(row[2 + 2 * i]) == boundary[b]
            pairs = [p.rsplit(":", 1) for p in row[3 + 2 * i].split(",")]
            assert [p[0] for p in pairs] == [names[u] for u in midx[mrow[b]:mrow[b + 1]]] and len(pairs) > 0
            assert [float(p[1]) for p in pairs] == list(mval[mrow[b]:mrow[b + 1]])
            b += 1
    assert b == len(boundary)

    lines = open(md, encoding="latin-1").read().split("\n")
    assert lines[-1] == ""
    rows = [l.split("\t") for l in lines[:-1]]
    assert [row[0] for row in rows] == want
    for s, row in enumerate(rows):
        assert float(row[1]) == score[s] and 0.0 < score[s] <= len(want[s])
        assert abs(float(row[2]) - plw[s]) <= 1e-14 * max(1.0, abs(plw[s]))   # %.15g
        assert [int(v) for v in row[3].split()] == list(pidx[prow[s]:prow[s + 1]])


@pytest.mark.parametrize("flag", ["-bm", "-md"])
def test_refused_without_an_automaton(flag, tmp_path):
    prefix = str(tmp_path / "m")
    r = subprocess.run([CLI, "-a", WFSA, "-c", CORPUS, "-opt", "QuasiNewton", "-e", "0", "-s", "-m", ">" + prefix],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = str(tmp_path / "out.tsv")
    r = subprocess.run([CLI, "-m", "<" + prefix, "-opt", "QuasiNewton", "-e", "1", "-i", "1", "-s", flag, out],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and flag + " needs an automaton and a corpus" in r.stderr
    assert not os.path.exists(out)


def test_usage_names_the_options():
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--byte-marginals FILE" in r.stderr and "--mea-decode FILE" in r.stderr
