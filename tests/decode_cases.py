"""The cases the decode tests share (test_gpu_best_paths.py,
test_gpu_kbest_paths.py): the golden and synthetic models, the oracle's
enumerated paths of each (oracle/hessian.py: the path-count matrix P and the
strings' path rows mrow), built once per session and left unchanged, and a
device that holds a case's whole corpus -- test infrastructure."""
import functools
import os

import numpy as np

from conftest import DATA

GOLDEN = [("talk", "talk"), ("test3", "test"), ("test5", "test5"), ("test5_2", "test5")]
# every string of these is recognized; paths counted by the CPU enumeration
FAMILIES = {
    # 51,242 paths, up to 823 per string
    "amb12": dict(n_states=12, degree=3, vocab=3, emissions=2, n_strings=150, max_len=8, seed=3),
    # compiled, 657 paths over 400 strings: most strings have fewer than 4
    "compiled64": dict(n_states=64, degree=4, vocab=16, emissions=1, n_strings=400, max_len=10, seed=3),
    # 202 nodes and ~400 in-edges per byte (more than three lane rounds of destinations), 4,283 paths
    "wide200": dict(n_states=200, degree=4, vocab=2, emissions=1, n_strings=60, max_len=6, seed=3),
    # lengths up to 64, 14,468 paths, exact ties present
    "long64": dict(n_states=64, degree=8, vocab=16, emissions=1, n_strings=300, max_len=64, seed=5),
    # amb12 at another seed, for the -inf case alone: with seed 3 (and 4, 12, 14, 15) the most-used
    # quarter of the parameters lies on every path, so no string keeps a finite one; with seed 7
    # (83,510 paths) 108 strings keep 1 .. 15 finite paths, 18 none and 24 at least 16 (CPU oracle)
    "amb12_seed7": dict(n_states=12, degree=3, vocab=3, emissions=2, n_strings=150, max_len=8, seed=7),
}


def _tol(v):
    return 1e-12 * max(1.0, abs(v))


@functools.lru_cache(maxsize=None)
def _golden(wfsa, corpus):
    import wfsa_amd as W
    text = open(os.path.join(DATA, wfsa + ".wfsa"), "rb").read().decode("latin-1")
    sym, off, wt = W.Corpus.read_file(os.path.join(DATA, corpus + ".corpus")).packed()
    return _reference(text, sym, off, wt)


@functools.lru_cache(maxsize=None)
def _family(name):
    import wfsa_amd as W
    syn = W.Synthetic(**FAMILIES[name])
    sym, off, wt = syn.corpus()
    return _reference(syn.wfsa_text, sym, off, wt)


def _source(name):
    for case in GOLDEN:
        if case[0] == name:
            return _golden(*case)
    return _family(name)


def _reference(text, sym, off, wt):
    """the oracle's path matrices, computed once per case and left unchanged"""
    from oracle import Oracle
    from oracle.hessian import HessianOracle
    o = Oracle.from_arrays(text, sym, off, wt)
    h = HessianOracle(o)
    return dict(text=text, sym=sym, off=off, wt=wt, o=o, h=h, P=h.P, mrow=np.asarray(h.mrow),
                rec=np.flatnonzero(o.path_counts() > 0), trim=o.trimmed_index())


def _device(ref, monkeypatch, tier2=False):
    """a device holding the WHOLE corpus (unrecognized strings included)"""
    import wfsa_amd as W
    monkeypatch.setenv("WFSA_TIER2", "1" if tier2 else "0")
    fsa = W.Fsa.read_text(ref["text"])
    dev = W.Device(0)
    dev.load_model(fsa)
    dev.load_corpus(ref["sym"], ref["off"], ref["wt"] / ref["wt"].sum())
    # the device numbers parameters as the reference does (its hash-map
    # order), the oracle by state order: match them by name
    names = {n: j for j, n in enumerate(ref["o"].full_param_names())}
    dev.perm = np.array([names[n] for n in fsa.param_names()], dtype=np.int64)
    return dev


def _big():
    import wfsa_amd as W
    syn = W.Synthetic(n_states=64, degree=8, vocab=16, emissions=1, n_strings=3000, max_len=64, seed=5)
    return (W.Fsa.read_text(syn.wfsa_text),) + tuple(syn.corpus())
