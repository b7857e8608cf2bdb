"""GPU tests of the Viterbi decode (wfsa_dev_best_paths, decode.hip): the
most probable accepting path of every string from the device's (max, +)
trellis pass with back-pointers, against the oracle's enumerated paths
(oracle/hessian.py: the path-count matrix P and the strings' path rows mrow).

Acceptance, for EVERY recognized string: best_logw equals max(P x) over the
string's paths within 1e-12 max(1, |value|) (the project's rmin tolerance; a
path sums at most ~70 terms of size ~1), the returned ids' counts equal the row
of SOME oracle path of the string whose weight is within that tolerance of the
max (the only allowance for ties), and the returned ids dotted with w_full
reproduce best_logw.  Needs a gfx950 device."""
import numpy as np
import pytest

from decode_cases import GOLDEN, _big, _device, _family, _golden, _tol

pytestmark = pytest.mark.gpu


def _accept(ref, x, perm, w_dev, logw, prow, pidx, strings):
    """the acceptance rule, for every recognized string; strings[r] = the
    index in (logw, prow) of the oracle's r-th recognized string"""
    P, mrow, trim = ref["P"], ref["mrow"], ref["trim"]
    lw = P @ x
    assert len(strings) == len(mrow) - 1
    for r, s in enumerate(strings):
        a, b = mrow[r], mrow[r + 1]
        want = lw[a:b].max()
        tol = _tol(want)
        assert abs(logw[s] - want) <= tol, (s, logw[s], want)
        ids = pidx[prow[s]:prow[s + 1]]
        assert abs(w_dev[ids].sum() - logw[s]) <= tol, (s, w_dev[ids].sum(), logw[s])
        t = trim[perm[ids]]
        assert (t != -2).all(), (s, ids)   # no unused parameter lies on a path
        row = np.bincount(t[t >= 0], minlength=P.shape[1])
        near = np.flatnonzero(np.abs(lw[a:b] - want) <= tol)
        assert any(np.array_equal(row, P[a + l]) for l in near), (s, ids)


def _check_device(ref, dev, seed):
    o = ref["o"]
    rng = np.random.default_rng(seed)
    n_all = len(ref["off"]) - 1
    out = []
    for _ in range(3):
        x = rng.normal(-1.0, 0.5, size=o.n)
        o.set_x(x)
        w = o.w_full()[dev.perm]
        logw, prow, pidx = dev.best_paths(w)
        assert logw.shape == (n_all,) and prow.shape == (n_all + 1,) and prow[0] == 0 and prow[-1] == len(pidx)
        _accept(ref, x, dev.perm, w, logw, prow, pidx, ref["rec"])
        miss = np.setdiff1d(np.arange(n_all), ref["rec"])   # unrecognized: -inf and an empty path
        assert np.all(np.isneginf(logw[miss])) and np.all(np.diff(prow)[miss] == 0)
        out.append((logw, prow, pidx))
    return out


@pytest.mark.parametrize("case", GOLDEN, ids=lambda c: c[0])
def test_best_paths_golden_cases(case, monkeypatch):
    """talk recognizes 3 of 5 strings, test3 4 of 7 (with exact ties and
    duplicate path rows); test5 repeats a parameter 9 times on a path"""
    ref = _golden(*case)
    n_all = len(ref["off"]) - 1
    if case[0] == "talk":
        assert (len(ref["rec"]), n_all) == (3, 5)
    if case[0] == "test3":
        assert (len(ref["rec"]), n_all) == (4, 7)
    _check_device(ref, _device(ref, monkeypatch), seed=5)


@pytest.mark.parametrize("name", ["amb12", "compiled64", "wide200", "long64"])
def test_best_paths_synthetic(name, monkeypatch):
    ref = _family(name)
    assert len(ref["rec"]) == len(ref["off"]) - 1   # every string recognized
    _check_device(ref, _device(ref, monkeypatch), seed=7)


@pytest.mark.parametrize("source", ["test3", "amb12"])
def test_best_paths_do_not_depend_on_the_tier(source, monkeypatch):
    """WFSA_TIER2=1 moves every string to the wide traversal kernel in the
    learning path; the decoder gives the same bytes"""
    ref = _golden("test3", "test") if source == "test3" else _family(source)
    auto = _check_device(ref, _device(ref, monkeypatch, tier2=False), seed=11)
    dev = _device(ref, monkeypatch, tier2=True)
    dev.recognize()
    if len(ref["rec"]) == len(ref["off"]) - 1:
        assert (dev.string_tiers() == 2).all()
    wide = _check_device(ref, dev, seed=11)
    for p, q in zip(auto, wide):
        for u, v in zip(p, q):
            assert u.tobytes() == v.tobytes()


def test_best_paths_repeat_byte_for_byte(monkeypatch):
    ref = _family("long64")
    dev = _device(ref, monkeypatch)
    o = ref["o"]
    o.set_x(np.random.default_rng(3).normal(-1.0, 0.5, size=o.n))
    w = o.w_full()[dev.perm]
    first = dev.best_paths(w)
    second = dev.best_paths(w)
    for u, v in zip(first, second):
        assert u.tobytes() == v.tobytes()
    assert dev.stats()["best_path_ms"] > 0.0


def test_decoder_leaves_the_quasinewton_loop_alone():
    """Run(3), Run(3) gives info rows bit-equal to Run(3), BestPaths(), Run(3)
    (rmin columns on)"""
    import wfsa_amd as W
    fsa, sym, off, wt = _big()
    runs = []
    for decode in (False, True):
        lrn = W.QuasiNewtonLearner(0)
        lrn.set_info_rmin(True)
        lrn.BuildFromPacked(fsa, sym, off, wt)
        lrn.Finalize()
        lrn.Init(7)
        rows = lrn.Run(3, 1.0, -1.0)
        if decode:
            logw, prow, pidx = lrn.BestPaths()
            assert np.isfinite(logw).all() and (np.diff(prow) > 0).all()
        rows += lrn.Run(3, 1.0, -1.0)
        runs.append(np.array(rows))
    assert runs[0].shape == (6, 7)
    assert runs[0].tobytes() == runs[1].tobytes()


def test_decoder_leaves_rmin_alone():
    """rmin() after objective_grad, best_paths(other weights) equals rmin()
    without the interleaved call"""
    import wfsa_amd as W
    fsa, sym, off, wt = _big()
    dev = W.Device(0)
    dev.load_model(fsa)
    dev.load_corpus(sym, off, wt / wt.sum())
    rng = np.random.default_rng(9)
    w1 = rng.normal(-1.0, 0.5, size=dev.n_params)
    w2 = rng.normal(-1.0, 0.5, size=dev.n_params)
    dev.objective_grad(w1, want_logq=False)
    plain = dev.rmin()
    assert plain[1] >= 0
    dev.objective_grad(w1, want_logq=False)
    dev.best_paths(w2)
    assert dev.rmin() == plain


@pytest.mark.parametrize("source", ["test3", "amb12"])
def test_learner_best_paths_after_a_device_run(source):
    """QuasiNewtonLearner.BestPaths() after run(flags=7, epochs=4) decodes at
    the state the device-resident loop left: the oracle at o.x() after the
    same four qn_steps"""
    import wfsa_amd as W
    ref = _golden("test3", "test") if source == "test3" else _family(source)
    o = ref["o"]
    fsa = W.Fsa.read_text(ref["text"])
    lrn = W.QuasiNewtonLearner(0)
    lrn.BuildFromPacked(fsa, ref["sym"], ref["off"], ref["wt"])
    lrn.Finalize()
    rows = lrn.run(flags=7, epochs=4)
    assert len(rows) == 4
    o.qn_init(7)
    for _ in range(4):
        o.qn_step(1.0)
    x = o.x()
    names = {n: j for j, n in enumerate(o.full_param_names())}
    perm = np.array([names[n] for n in fsa.param_names()], dtype=np.int64)
    tw = lrn.trimmed_index()
    w_dev = np.where(tw >= 0, np.append(lrn.x(), 0.0)[tw], np.where(tw == -1, 0.0, -np.inf))   # GetWeight
    logw, prow, pidx = lrn.BestPaths()
    n_local = lrn.info()["n_local_strings"]
    assert logw.shape == (n_local,) and n_local == len(ref["rec"])
    _accept(ref, x, perm, w_dev, logw, prow, pidx, np.arange(n_local))
    # HessianLearner inherits the method
    assert W.HessianLearner.BestPaths is W.QuasiNewtonLearner.BestPaths


def test_best_paths_errors(monkeypatch):
    import wfsa_amd as W
    from wfsa_amd import _lib
    ref = _golden("talk", "talk")
    fsa = W.Fsa.read_text(ref["text"])
    # before a corpus is loaded
    dev = W.Device(0)
    with pytest.raises(W.WfsaError) as e:
        dev.best_paths(np.zeros(0))
    assert e.value.code == _lib.WFSA_ERR_ARG
    dev.load_model(fsa)
    with pytest.raises(W.WfsaError) as e:
        dev.best_paths(np.zeros(dev.n_params))
    assert e.value.code == _lib.WFSA_ERR_ARG
    # while an evaluation is in flight
    dev.load_corpus(ref["sym"], ref["off"], ref["wt"] / ref["wt"].sum())
    w = np.full(dev.n_params, -1.0)
    dev.objective_grad_begin(w)
    with pytest.raises(W.WfsaError) as e:
        dev.best_paths(w)
    assert e.value.code == _lib.WFSA_ERR_ARG and "in flight" in str(e.value)
    dev.objective_grad_end()
    logw, _, _ = dev.best_paths(w)
    assert np.isfinite(logw).sum() == 3
    # matrix-file mode: no automaton
    dev.load_paths(2, [0, 1, 2], [0, 1], [1.0, 1.0], [0, 2], [0, 1], [1.0])
    with pytest.raises(W.WfsaError) as e:
        dev.best_paths(np.zeros(2))
    assert e.value.code == _lib.WFSA_ERR_ARG and "matrix" in str(e.value)
    # the dense path builds no trellis
    monkeypatch.setenv("WFSA_DENSE", "1")
    syn = W.Synthetic(n_states=16, degree=1, vocab=6, emissions=2, dense=True, n_strings=50, max_len=9, seed=3)
    sym, off, wt = syn.corpus()
    dd = W.Device(0)
    dd.load_model(W.Fsa.read_text(syn.wfsa_text))
    dd.load_corpus(sym, off, wt / wt.sum())
    assert dd.stats()["dense"] == 1
    with pytest.raises(W.WfsaError) as e:
        dd.best_paths(np.full(dd.n_params, -1.0))
    assert e.value.code == _lib.WFSA_ERR_CAPACITY and "WFSA_DENSE=0" in str(e.value)
