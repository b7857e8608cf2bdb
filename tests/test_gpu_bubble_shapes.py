"""Small-bubble sweeps compiled for the bubbles' structures (fb_kernels.hip
small_bubble: shaped_sweeps, the turns over a wave's structure ids, the sums
and stores after them).

A structure with compiled-in sweeps runs the operations of the generic
select-tree sweeps in the same order, so every result keeps its bits:
WFSA_BUBBLE_SHAPES=0 (every structure id 0, every lane on the generic turn)
and the default must agree bit for bit -- KL and gradient, log q (through
bubble_kernel), the rows, x and the last gradient of a device-resident run on
both step paths, and the rmin columns.  The per-structure sweeps run in
step_dot_kernel without the rmin column; bubble_kernel and the rmin variants
keep the generic sweeps and read the same table headers, ids included.  One
case checks the default against the ENUM oracle, since both settings could be
wrong together.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CORPORA = {
    # a few dozen class-A waves, a handful of class-B waves, a partial last wave in each class
    "familyA20k": dict(n_states=1024, degree=8, vocab=64, emissions=1, n_strings=20_000, max_len=128, seed=1),
    # many structures: waves of several structure ids, listed and unlisted structures side by side
    "ambiguous": dict(n_states=256, degree=8, vocab=16, emissions=1, n_strings=8_000, max_len=64, seed=4,
                      compiled_only=True),
    # the class-B list shorter than one wave: inactive lanes beside grouped lanes
    "familyA300": dict(n_states=1024, degree=8, vocab=64, emissions=1, n_strings=300, max_len=128, seed=1),
}


@functools.lru_cache(maxsize=None)
def _corpus(name):
    import wfsa_amd as W
    kw = dict(CORPORA[name])
    compiled_only = kw.pop("compiled_only", False)
    syn = W.Synthetic(**kw)
    sym, off, wt = syn.corpus()
    fsa = W.Fsa.read_text(syn.wfsa_text)
    if compiled_only:   # the strings that compile (the others make the loop take the separate kernel)
        dev = W.Device(0)
        dev.load_model(fsa)
        dev.load_corpus(sym, off, wt / wt.sum())
        dev.recognize()
        dev.objective_grad(np.full(len(fsa.param_names()), -1.0), want_logq=False)
        keep = np.flatnonzero(dev.string_tiers() < 0)
        lens = np.diff(off)[keep]
        sym = np.concatenate([sym[off[i]:off[i + 1]] for i in keep]).astype(np.uint8)
        off, wt = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), wt[keep]
    return syn.wfsa_text, fsa, sym, off, wt


def _learner(name, monkeypatch, shapes, inkernel=None, rmin=False):
    import wfsa_amd as W
    _, fsa, sym, off, wt = _corpus(name)
    if shapes:
        monkeypatch.delenv("WFSA_BUBBLE_SHAPES", raising=False)
    else:
        monkeypatch.setenv("WFSA_BUBBLE_SHAPES", "0")
    if inkernel is None:
        monkeypatch.delenv("WFSA_QN_INKERNEL", raising=False)
    else:
        monkeypatch.setenv("WFSA_QN_INKERNEL", "1" if inkernel else "0")
    lrn = W.QuasiNewtonLearner(0)
    lrn.set_info_rmin(rmin)
    lrn.BuildFromPacked(fsa, sym, off, wt)
    lrn.Finalize()
    lrn.Init(7)
    return lrn


def _counts(lrn):
    """(small bubbles with a compiled-in structure, waves of several structure
    ids, class-A small bubbles, class-B small bubbles)"""
    st = lrn.stats()
    return st["shaped_bubbles"], st["mixed_shape_waves"], st["small_bubbles_a"], st["small_bubbles_b"]


@pytest.mark.parametrize("name", sorted(CORPORA))
def test_objective_grad_bits(name, monkeypatch):
    """KL and the gradient (step_dot_kernel without the QN update: the
    per-structure sweeps against the generic ones), then log q (bubble_kernel,
    the per-bubble log Z form: it keeps the generic sweeps, so this half
    shows that it masks the ids out of the headers it reads)"""
    a = _learner(name, monkeypatch, True)
    b = _learner(name, monkeypatch, False)
    print(f"{name}: (compiled-in, mixed waves, class A, class B) default {_counts(a)} knob off {_counts(b)}")
    for want_logq in (False, True):
        kl_a, g_a, lq_a = a.objective_grad(want_logq=want_logq)
        kl_b, g_b, lq_b = b.objective_grad(want_logq=want_logq)
        assert kl_a == kl_b, (want_logq, kl_a, kl_b)
        assert np.array_equal(g_a, g_b), (want_logq, np.flatnonzero(g_a != g_b)[:8])
        if want_logq:
            assert np.isfinite(lq_a).all()
            assert np.array_equal(lq_a, lq_b), np.flatnonzero(lq_a != lq_b)[:8]


@pytest.mark.parametrize("rmin", [False, True], ids=["", "rmin"])
@pytest.mark.parametrize("inkernel", [True, False], ids=["one_launch", "two_kernels"])
@pytest.mark.parametrize("name", sorted(CORPORA))
def test_run_bits(name, inkernel, rmin, monkeypatch):
    """five device-resident steps: the rows, x and the last gradient.  With
    rmin the rows' columns 5 and 6 too -- but the rmin variants of the step
    kernel keep the generic sweeps (the per-structure form spills there), so
    those cases run the same sweeps on both sides: they show that the ids in
    the table headers are masked wherever the header is read (the (min, x)
    pass compares headers), not a (min, x) pass after specialised sweeps,
    which no kernel has"""
    a = _learner(name, monkeypatch, True, inkernel, rmin)
    b = _learner(name, monkeypatch, False, inkernel, rmin)
    ra, rb = np.array(a.Run(5, 1.0, -1.0)), np.array(b.Run(5, 1.0, -1.0))
    assert ra.shape == rb.shape and ra.shape[0] == 5
    assert np.isfinite(ra[:, :5]).all()
    assert np.array_equal(ra, rb), [(int(r), int(c), ra[r, c], rb[r, c]) for r, c in np.argwhere(ra != rb)[:8]]
    assert np.array_equal(a.x(), b.x())
    assert np.array_equal(a.last_grad(), b.last_grad())
    assert (a.stats()["qn_inkernel_waves"] > 0) == (b.stats()["qn_inkernel_waves"] > 0)   # (the same step path)


def test_counters_and_knob(monkeypatch):
    """the corpora reach the branches they are here for, and the knob reaches the tables"""
    for name in sorted(CORPORA):
        shaped, mixed, n_a, n_b = _counts(_learner(name, monkeypatch, True))
        shaped0, mixed0, n_a0, n_b0 = _counts(_learner(name, monkeypatch, False))
        print(f"{name}: small bubbles class A {n_a} class B {n_b}, with a compiled-in structure {shaped}, "
              f"waves of several ids {mixed}; knob off: {shaped0}, {mixed0}")
        assert (n_a, n_b) == (n_a0, n_b0) and n_a > 0 and n_b > 0
        assert shaped0 == 0 and mixed0 == 0
        assert 0 < shaped <= n_a + n_b
        if name == "familyA20k":   # whole waves and a partial last wave in each class
            assert n_a > 64 and n_a % 64 != 0 and n_b > 64 and n_b % 64 != 0, (n_a, n_b)
        if name == "ambiguous":
            assert mixed > 0, "no wave runs more than one turn"
            assert shaped < n_a + n_b, "no small bubble has id 0: the generic turn never runs beside specialised ones"
        if name == "familyA300":   # the class-B list shorter than one wave: inactive lanes beside grouped lanes
            assert 0 < n_b < 64, n_b


def test_default_matches_enum_oracle(monkeypatch):
    """family A, 20,000 strings, the default setting against the reference's
    path enumeration: log q and the gradient at tests/test_gpu_parity.py's
    tolerances for them"""
    from oracle import ENUM, Oracle
    text, fsa, sym, off, wt = _corpus("familyA20k")
    lrn = _learner("familyA20k", monkeypatch, True)
    assert lrn.stats()["shaped_bubbles"] > 0
    o = Oracle.from_arrays(text, sym, off, wt, mode=ENUM, max_paths=10_000_000)
    o.set_threads(8)
    assert lrn.info()["n_params"] == o.info["n_params"] and lrn.info()["n_paths"] == o.info["n_paths"]
    o.qn_init(7)   # (the learner's Init(7): the same initial weights)
    x = dict(zip(lrn.param_names(), lrn.x()))
    on = o.param_names()
    assert set(on) == set(x)
    np.testing.assert_allclose([x[k] for k in on], o.x(), rtol=1e-13, atol=0)
    o.objective_grad()
    _, grad, logq = lrn.objective_grad(want_logq=True)
    g = dict(zip(lrn.param_names(), grad))
    ologq = o.logq()
    assert logq.shape == ologq.shape
    np.testing.assert_allclose(logq, ologq, rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose([g[k] for k in on], o.grad(), rtol=1e-10, atol=1e-15)
