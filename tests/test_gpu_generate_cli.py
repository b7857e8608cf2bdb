"""GPU test of the CLI's -gen N FILE (main.cpp): without -c nothing is learned
and the automaton's weights as read drive the walk; FILE is a corpus (separator
TAB) of the distinct complete strings with their counts, equal to
Device.generate(...).distinct() for the same seed; another seed gives another
file and the same call the same file.  Needs a gfx950 device."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from decode_cases import _family

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "w-fsa_amd", "wfsa_amd", "wfsa")


def _run(args):
    r = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


@pytest.mark.parametrize("flag", ["-gen", "--generate"])
def test_generate_file_matches_the_device(flag, tmp_path):
    import wfsa_amd as W
    model = str(tmp_path / "amb12.wfsa")
    open(model, "wb").write(_family("amb12")["text"].encode("latin-1"))
    out, again, other = str(tmp_path / "g.corpus"), str(tmp_path / "again.corpus"), str(tmp_path / "other.corpus")
    err = _run(["-a", model, flag, "2000", out, "--gen-max-len", "8"])
    assert open(out, "rb").read().startswith(b"\t\n")

    fsa = W.Fsa.read_file(model)
    dev = W.Device(0)
    dev.load_model(fsa)
    got = dev.generate(fsa.weights(), 2000, max_len=8, seed=0)
    sym, off, counts = got.distinct()
    want = [(sym[off[s]:off[s + 1]].tobytes().decode("latin-1"), counts[s]) for s in range(len(counts))]
    # (amb12's bytes are digits: every complete string but the empty one can be written)
    writable = [(s, c) for s, c in want if s]
    strings, weights = W.Corpus.read_file(out).strings()
    assert list(zip(strings, weights)) == writable
    complete = int((got["status"] == 0).sum())
    assert weights.sum() == complete - sum(c for s, c in want if not s) > 0
    assert "complete: %d" % complete in err and "truncated: %d" % int((got["status"] == 1).sum()) in err

    # the same call: the same file; another seed: other draws
    _run(["-a", model, flag, "2000", again, "--gen-max-len", "8"])
    assert open(out, "rb").read() == open(again, "rb").read()
    _run(["-a", model, flag, "2000", other, "--gen-max-len", "8", "--sample-seed", "77"])
    assert open(out, "rb").read() != open(other, "rb").read()
    sym, off, counts = dev.generate(fsa.weights(), 2000, max_len=8, seed=77).distinct()
    strings, weights = W.Corpus.read_file(other).strings()
    assert strings == [sym[off[s]:off[s + 1]].tobytes().decode("latin-1") for s in range(len(counts)) if off[s + 1] > off[s]]


def test_generate_after_learning_uses_the_final_weights(tmp_path):
    """with -c and epochs: the Python learner taking the same steps generates the same strings"""
    import wfsa_amd as W
    from conftest import DATA
    wfsa, corpus = os.path.join(DATA, "test3.wfsa"), os.path.join(DATA, "test.corpus")
    out = str(tmp_path / "g.corpus")
    _run(["-a", wfsa, "-c", corpus, "-opt", "QuasiNewton", "-e", "3", "-i", "1", "-s", "-gen", "500", out, "--gen-max-len", "6",
          "--sample-seed", "5"])
    lrn = W.QuasiNewtonLearner(0)
    lrn.BuildFrom(W.Fsa.read_file(wfsa), W.Corpus.read_file(corpus))
    lrn.Finalize()
    lrn.Init(1)
    for _ in range(3):   # the CLI's epoch loop: eta 1, tol 1e-6
        _, halt = lrn.OptimizationStep(1.0, 1e-6)
        if halt:
            break
    sym, off, counts = lrn.Generate(500, max_len=6, seed=5).distinct()
    strings, weights = W.Corpus.read_file(out).strings()
    keep = [s for s in range(len(counts)) if off[s + 1] > off[s]]
    assert strings == [sym[off[s]:off[s + 1]].tobytes().decode("latin-1") for s in keep] and len(strings) > 0
    assert list(weights) == [counts[s] for s in keep]


def test_usage_names_the_option():
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--generate N FILE" in r.stderr and "--gen-max-len L" in r.stderr
