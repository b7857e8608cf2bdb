"""The step launch without the stream pass (fb_kernels.hip step_dot_kernel).

An evaluation that does not want log q needs the stream pass only for the
log-likelihood, and the trivial words' share of it is a dot product: sum_s
p_s sum_{j in trivial(s)} w_j = -sum_j g_j w_j with g the rank's own
trivial-word gradient, constant for a prepared corpus (qn_device.hpp
ll_trivial_share).  So the step launches bubbles, arrival and QN waves alone.
Against the stream pass (WFSA_LL_DOT=0, and the evaluation with log q, which
keeps it) the gradient, x, the trajectory and every info column but KL are
the same bits; KL is the same sum reassociated (rel 1e-12, atol 1e-13: the
bound of the same sum reassociated across ranks, test_gpu_multiprocess.py).
A parameter Trim dropped has weight -inf and coefficient 0: its term must be
selected away, not multiplied (the sparse-use shape).
"""
import json
import math
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "ll_dot_oracle.json")

SHAPES = {
    "A-small": dict(n_states=256, degree=8, vocab=64, emissions=1, n_strings=20_000, max_len=64, seed=1),
    # test_gpu_qn_inkernel's: many bubbles per string, popular parameters
    "ambiguous": dict(n_states=256, degree=8, vocab=16, emissions=1, n_strings=8_000, max_len=64, seed=4,
                      compiled_only=True),
    # strings that do not compile, on the traversal kernels
    "traversal": dict(n_states=1024, degree=8, vocab=16, emissions=4, n_strings=3_000, max_len=128, seed=2),
    # few strings: parameters no string uses are trimmed (weight -inf)
    "sparse-use": dict(n_states=256, degree=8, vocab=64, emissions=1, n_strings=300, max_len=32, seed=1),
}
ENUMERATES = {"A-small", "ambiguous", "sparse-use"}   # ENUM there, TRELLIS for the traversal shape
ALL = sorted(SHAPES)


def _close(a, b, rel=1e-12, atol=1e-13):
    return abs(a - b) <= max(atol, rel * max(abs(a), abs(b)))


_corpora = {}


@pytest.fixture(scope="module", autouse=True)
def _release_corpora():
    yield
    _corpora.clear()   # (the model handles go before the interpreter shuts down)


def _corpus(W, shape):
    """(fsa, sym, off, wt) of a shape, built once per session"""
    if shape in _corpora:
        return _corpora[shape]
    kw = dict(SHAPES[shape])
    compiled_only = kw.pop("compiled_only", False)
    syn = W.Synthetic(**kw)
    sym, off, wt = syn.corpus()
    fsa = W.Fsa.read_text(syn.wfsa_text)
    if compiled_only:   # the strings that compile, as test_gpu_qn_inkernel.py takes them
        dev = W.Device(0)
        dev.load_model(fsa)
        dev.load_corpus(sym, off, wt / wt.sum())
        dev.recognize()
        dev.objective_grad(np.full(len(fsa.param_names()), -1.0), want_logq=False)
        keep = np.flatnonzero(dev.string_tiers() < 0)
        lens = np.diff(off)[keep]
        off_k = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        sym = np.concatenate([sym[off[i]:off[i + 1]] for i in keep]).astype(np.uint8)
        off, wt = off_k, wt[keep]
    _corpora[shape] = (syn.wfsa_text, fsa, sym, off, wt)
    return _corpora[shape]


_oracle_kl = {}


def _oracle(W, shape):
    """the oracle's KL at Init(7), once per shape.  The traversal shape's
    dense TRELLIS pass takes about a minute on one core, so its value is a
    recorded fixture (tests/golden/ll_dot_oracle.json, written from the code
    below with the entry removed)"""
    if shape not in _oracle_kl:
        rec = json.load(open(GOLDEN)).get(shape)
        if rec is not None:
            want = {k: v for k, v in SHAPES[shape].items() if k != "compiled_only"}
            assert rec["shape"] == want, "the recorded oracle value is for another shape"
            _oracle_kl[shape] = rec["kl_init7"]
            return _oracle_kl[shape]
        from oracle import ENUM, TRELLIS, Oracle
        text, _, sym, off, wt = _corpus(W, shape)
        mode = ENUM if shape in ENUMERATES else TRELLIS
        o = Oracle.from_arrays(text, sym, off, wt, mode=mode, max_paths=10_000_000)
        o.qn_init(7)
        _oracle_kl[shape] = o.objective_grad()[0]
    return _oracle_kl[shape]


def _learner(W, shape, monkeypatch, dot=True, inkernel=True, rmin=False):
    _, fsa, sym, off, wt = _corpus(W, shape)
    monkeypatch.setenv("WFSA_QN_INKERNEL", "1" if inkernel else "0")
    monkeypatch.setenv("WFSA_LL_DOT", "1" if dot else "0")
    lrn = W.QuasiNewtonLearner(0)
    lrn.set_info_rmin(rmin)
    lrn.BuildFromPacked(fsa, sym, off, wt)
    lrn.Finalize()
    lrn.Init(7)
    return lrn


@pytest.mark.parametrize("shape", ALL)
def test_dot_evaluation_against_the_stream_pass_and_the_oracle(shape, monkeypatch):
    import wfsa_amd as W
    a = _learner(W, shape, monkeypatch)
    if shape == "sparse-use":   # else the shape proves nothing about the -inf guard
        assert (a.trimmed_index() == -2).any(), "no parameter was trimmed as unused"
    kl, g, _ = a.objective_grad()
    assert a.stats()["ll_dot_launches"] > 0, "the stream-less launch did not run"
    kl_q, g_q, logq = a.objective_grad(want_logq=True)   # (keeps the stream pass)
    p = a.p()
    kl_p = math.fsum(t * math.log(t) for t in p if t > 0.0) - math.fsum(p * logq)
    kl_o = _oracle(W, shape)
    print(f"{shape}: KL dot {kl!r}, stream {kl_q!r} (rel {abs(kl - kl_q) / abs(kl_q):.2e}), "
          f"plogp - p.logq {kl_p!r}, oracle {kl_o!r} (rel {abs(kl - kl_o) / abs(kl_o):.2e})")
    assert math.isfinite(kl)
    assert np.array_equal(g, g_q)
    assert _close(kl, kl_q)
    assert _close(kl, kl_p)
    assert _close(kl, kl_o, rel=1e-11)
    # the knob off: the stream pass everywhere
    b = _learner(W, shape, monkeypatch, dot=False)
    kl_b, g_b, _ = b.objective_grad()
    b.Run(2, 1.0, -1.0)
    assert b.stats()["ll_dot_launches"] == 0
    assert np.array_equal(g, g_b) and _close(kl, kl_b)


@pytest.mark.parametrize("rmin", [False, True], ids=["", "rmin"])
@pytest.mark.parametrize("shape", ALL)
def test_run_equals_the_stream_pass_run(shape, rmin, monkeypatch):
    """the log-likelihood feeds no update: x, the gradient and every column
    but KL are the stream pass's bits"""
    import wfsa_amd as W
    a = _learner(W, shape, monkeypatch, rmin=rmin)
    b = _learner(W, shape, monkeypatch, dot=False, rmin=rmin)
    ra, rb = np.array(a.Run(7, 1.0, -1.0)), np.array(b.Run(7, 1.0, -1.0))
    assert a.stats()["ll_dot_launches"] > 0 and b.stats()["ll_dot_launches"] == 0
    assert a.stats()["qn_inkernel_waves"] == b.stats()["qn_inkernel_waves"]   # (the same path choice)
    print(f"{shape}: KL column max rel diff {np.max(np.abs(ra[:, 0] - rb[:, 0]) / np.abs(rb[:, 0])):.2e}")
    np.testing.assert_array_equal(a.x(), b.x())
    np.testing.assert_array_equal(a.last_grad(), b.last_grad())
    assert ra.shape == rb.shape == (7, ra.shape[1])
    np.testing.assert_array_equal(ra[:, 1:5], rb[:, 1:5])
    if rmin:
        np.testing.assert_array_equal(ra[:, 5:7], rb[:, 5:7])
    assert np.isfinite(ra[:, 0]).all()
    for u, v in zip(ra[:, 0], rb[:, 0]):
        assert _close(u, v), (u, v)


@pytest.mark.parametrize("rmin", [False, True], ids=["", "rmin"])
@pytest.mark.parametrize("shape", ["A-small", "sparse-use"])
def test_inkernel_step_equals_separate_kernel_step(shape, rmin, monkeypatch):
    """both steps and objective_grad launch the same stream-less kernel
    geometry: the same partials in the same ll_part slots, KL included"""
    import wfsa_amd as W
    a = _learner(W, shape, monkeypatch, inkernel=True, rmin=rmin)
    b = _learner(W, shape, monkeypatch, inkernel=False, rmin=rmin)
    ra = a.Run(3, 1.0, -1.0) + a.Run(4, 1.0, -1.0)
    rb = b.Run(7, 1.0, -1.0)
    if shape == "A-small":
        assert a.stats()["qn_inkernel_waves"] > 0, "the in-kernel update did not run"
    assert b.stats()["qn_inkernel_waves"] == 0
    assert a.stats()["ll_dot_launches"] > 0 and b.stats()["ll_dot_launches"] > 0
    np.testing.assert_array_equal(np.array(ra), np.array(rb))
    np.testing.assert_array_equal(a.x(), b.x())
    np.testing.assert_array_equal(a.last_grad(), b.last_grad())
    kl_a, g_a, _ = a.objective_grad()
    kl_b, g_b, _ = b.objective_grad()
    assert kl_a == kl_b and np.array_equal(g_a, g_b)


@pytest.mark.parametrize("shape", ALL)
def test_dot_path_repeats_bit_for_bit(shape, monkeypatch):
    """two runs, and a second fresh context (its own preparation-time
    coefficients), give the same bits"""
    import wfsa_amd as W
    a = _learner(W, shape, monkeypatch)
    kl_a, g_a, _ = a.objective_grad()
    kl_a2, g_a2, _ = a.objective_grad()
    assert kl_a == kl_a2 and np.array_equal(g_a, g_a2)
    runs = []
    for _ in range(2):
        a.Init(7)
        rows = a.Run(6, 1.0, -1.0)
        runs.append((np.array(rows), a.x(), a.last_grad()))
    for u, v in zip(runs[0], runs[1]):
        np.testing.assert_array_equal(u, v)
    b = _learner(W, shape, monkeypatch)
    kl_b, g_b, _ = b.objective_grad()
    assert kl_b == kl_a and np.array_equal(g_b, g_a)
    rows_b = np.array(b.Run(6, 1.0, -1.0))
    np.testing.assert_array_equal(rows_b, runs[0][0])
    np.testing.assert_array_equal(b.x(), runs[0][1])
