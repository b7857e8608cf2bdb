"""GPU tests of what the eight per-string entry points and their ten getters say
when they refuse a call: the error code, the full message and which check
speaks first.  The entry points are wfsa_dev_best_paths, _kbest_paths,
_sample_paths, _posterior_counts and _byte_marginals on the trellis tiers and
wfsa_dev_dense_best_paths, _dense_sample_paths and _dense_byte_marginals on the
dense path.  Every expected message is written out in full here; none is put
together the way the library does it.  The model is the 16-state case of
dense_decode_reference.py, loaded once with WFSA_DENSE=1 and once with
WFSA_DENSE=0.  Needs a gfx950 device."""
import numpy as np
import pytest

import dense_decode_reference as R

pytestmark = pytest.mark.gpu

ARG, CAPACITY = -1, -4   # WFSA_ERR_ARG, WFSA_ERR_CAPACITY (wfsa_dev.h)
TRELLIS = ("best_paths", "kbest_paths", "sample_paths", "posterior_counts", "byte_marginals")
DENSE = ("dense_best_paths", "dense_sample_paths", "dense_byte_marginals")

MATRIX = {
    "best_paths": "best_paths: matrix-file mode has no automaton to decode over",
    "kbest_paths": "kbest_paths: matrix-file mode has no automaton to decode over",
    "sample_paths": "sample_paths: matrix-file mode has no automaton to sample over",
    "posterior_counts": "posterior_counts: matrix-file mode has no automaton to walk",
    "byte_marginals": "byte_marginals: matrix-file mode has no automaton to walk",
    "dense_best_paths": "dense_best_paths: matrix-file mode has no automaton to decode over",
    "dense_sample_paths": "dense_sample_paths: matrix-file mode has no automaton to sample over",
    "dense_byte_marginals": "dense_byte_marginals: matrix-file mode has no automaton to walk",
}
NOT_LOADED = {
    "best_paths": "best_paths: load a model and a corpus first",
    "kbest_paths": "kbest_paths: load a model and a corpus first",
    "sample_paths": "sample_paths: load a model and a corpus first",
    "posterior_counts": "posterior_counts: load a model and a corpus first",
    "byte_marginals": "byte_marginals: load a model and a corpus first",
    "dense_best_paths": "dense_best_paths: load a model and a corpus first",
    "dense_sample_paths": "dense_sample_paths: load a model and a corpus first",
    "dense_byte_marginals": "dense_byte_marginals: load a model and a corpus first",
}
IN_FLIGHT = {
    "best_paths": "best_paths: an evaluation is in flight",
    "kbest_paths": "kbest_paths: an evaluation is in flight",
    "sample_paths": "sample_paths: an evaluation is in flight",
    "posterior_counts": "posterior_counts: an evaluation is in flight",
    "byte_marginals": "byte_marginals: an evaluation is in flight",
    "dense_best_paths": "dense_best_paths: an evaluation is in flight",
    "dense_sample_paths": "dense_sample_paths: an evaluation is in flight",
    "dense_byte_marginals": "dense_byte_marginals: an evaluation is in flight",
}
WRONG_TIER = {
    "best_paths": (CAPACITY, "best_paths: the dense path builds no trellis; load the model with WFSA_DENSE=0 to decode it"),
    "kbest_paths": (CAPACITY, "kbest_paths: the dense path builds no trellis; load the model with WFSA_DENSE=0 to decode it"),
    "sample_paths": (CAPACITY, "sample_paths: the dense path builds no trellis; load the model with WFSA_DENSE=0 to sample it"),
    "posterior_counts": (CAPACITY, "posterior_counts: the dense path builds no trellis; load the model with WFSA_DENSE=0 to take its posterior"),
    "byte_marginals": (CAPACITY, "byte_marginals: the dense path builds no trellis; load the model with WFSA_DENSE=0 to take its marginals"),
    "dense_best_paths": (ARG, "dense_best_paths: the model is not on the dense path; decode it with wfsa_dev_best_paths"),
    "dense_sample_paths": (ARG, "dense_sample_paths: the model is not on the dense path; sample it with wfsa_dev_sample_paths"),
    "dense_byte_marginals": (ARG, "dense_byte_marginals: the model is not on the dense path; take its marginals with wfsa_dev_byte_marginals"),
}
NAN = {
    "dense_best_paths": "dense_best_paths: a weight is NaN or +inf",
    "dense_sample_paths": "dense_sample_paths: a weight is NaN or +inf",
    "dense_byte_marginals": "dense_byte_marginals: a weight is NaN or +inf",
}
# the argument each entry point checks between the state and the tier, at values it refuses
BAD_ARG = {
    "kbest_paths": [(dict(k=0), "kbest_paths: k = 0 is outside 1 .. 16"), (dict(k=17), "kbest_paths: k = 17 is outside 1 .. 16")],
    "sample_paths": [(dict(n=0), "sample_paths: n = 0 is outside 1 .. 64"), (dict(n=65), "sample_paths: n = 65 is outside 1 .. 64")],
    "dense_sample_paths": [(dict(n=0), "dense_sample_paths: n = 0 is outside 1 .. 64"),
                           (dict(n=65), "dense_sample_paths: n = 65 is outside 1 .. 64")],
    "dense_byte_marginals": [(dict(rows=0, decode=0), "dense_byte_marginals: rows = 0 and decode = 0 ask for nothing")],
}
NO_RESULT = {
    "best_paths_get": "best_paths_get: no wfsa_dev_best_paths result since the last load",
    "kbest_paths_get": "kbest_paths_get: no wfsa_dev_kbest_paths result since the last load",
    "sample_paths_get": "sample_paths_get: no wfsa_dev_sample_paths result since the last load",
    "posterior_counts_get": "posterior_counts_get: no wfsa_dev_posterior_counts result since the last load",
    "byte_marginals_get": "byte_marginals_get: no wfsa_dev_byte_marginals result since the last load",
    "byte_marginals_path_get": "byte_marginals_path_get: no wfsa_dev_byte_marginals result since the last load",
    "dense_best_paths_get": "dense_best_paths_get: no wfsa_dev_dense_best_paths result since the last load",
    "dense_sample_paths_get": "dense_sample_paths_get: no wfsa_dev_dense_sample_paths result since the last load",
    "dense_byte_marginals_get": "dense_byte_marginals_get: no wfsa_dev_dense_byte_marginals result since the last load",
    "dense_byte_marginals_path_get": "dense_byte_marginals_path_get: no wfsa_dev_dense_byte_marginals result since the last load",
}
GETTERS = {"best_paths_get": 2, "kbest_paths_get": 4, "sample_paths_get": 4, "posterior_counts_get": 3, "byte_marginals_get": 3,
           "byte_marginals_path_get": 2, "dense_best_paths_get": 2, "dense_sample_paths_get": 4, "dense_byte_marginals_get": 3,
           "dense_byte_marginals_path_get": 2}   # name: output pointers


def _lib():
    from wfsa_amd import _lib as L
    return L.load()


def _call(dev, name, w, k=4, n=2, rows=1, decode=1):
    """(code, message) of one raw call of wfsa_dev_<name>; w None: null weights.
    Every output pointer is null: the entry points take that."""
    lib, h = _lib(), dev._h
    wp = None if w is None else w.ctypes.data
    rc = {
        "best_paths": lambda: lib.wfsa_dev_best_paths(h, wp, None, None),
        "kbest_paths": lambda: lib.wfsa_dev_kbest_paths(h, wp, k, None, None),
        "sample_paths": lambda: lib.wfsa_dev_sample_paths(h, wp, n, 7, None, None, None),
        "posterior_counts": lambda: lib.wfsa_dev_posterior_counts(h, wp, None, None, None),
        "byte_marginals": lambda: lib.wfsa_dev_byte_marginals(h, wp, decode, None, None, None, None, None, None),
        "dense_best_paths": lambda: lib.wfsa_dev_dense_best_paths(h, wp, None, None),
        "dense_sample_paths": lambda: lib.wfsa_dev_dense_sample_paths(h, wp, n, 7, None, None, None),
        "dense_byte_marginals": lambda: lib.wfsa_dev_dense_byte_marginals(h, wp, rows, decode, None, None, None, None, None),
    }[name]()
    return rc, (lib.wfsa_dev_last_error().decode() if rc else "")


def _get(dev, getter):
    """(code, message) of a getter called with null outputs"""
    lib = _lib()
    rc = getattr(lib, "wfsa_dev_" + getter)(dev._h, *([None] * GETTERS[getter]))
    return rc, (lib.wfsa_dev_last_error().decode() if rc else "")


def _case():
    import wfsa_amd as W
    text, sym, off, wt = R.synthetic("dense16")
    fsa = W.Fsa.read_text(text)
    return fsa, sym, off, wt / wt.sum(), R.case_weights("dense16", len(fsa.param_names()))


def _device(monkeypatch, dense, corpus=True):
    import wfsa_amd as W
    fsa, sym, off, p, _ = _case()
    monkeypatch.setenv("WFSA_DENSE", "1" if dense else "0")
    dev = W.Device(0)
    dev.load_model(fsa)
    if corpus:
        dev.load_corpus(sym, off, p)
        assert dev.stats()["dense"] == (1 if dense else 0)
    return dev


def test_nothing_loaded_and_model_without_corpus(monkeypatch):
    import wfsa_amd as W
    empty = W.Device(0)
    for name in TRELLIS + DENSE:
        assert _call(empty, name, np.zeros(1)) == (ARG, NOT_LOADED[name])
    for dense in (True, False):
        dev = _device(monkeypatch, dense, corpus=False)
        for name in TRELLIS + DENSE:
            assert _call(dev, name, np.zeros(dev.n_params)) == (ARG, NOT_LOADED[name])


@pytest.mark.parametrize("dense", [True, False])
def test_evaluation_in_flight_speaks_before_the_arguments(dense, monkeypatch):
    w = _case()[4]
    dev = _device(monkeypatch, dense)
    dev.recognize()
    dev.objective_grad_begin(w)
    try:
        for name in TRELLIS + DENSE:
            assert _call(dev, name, w) == (ARG, IN_FLIGHT[name])
            for bad, _ in BAD_ARG.get(name, []):
                assert _call(dev, name, w, **bad) == (ARG, IN_FLIGHT[name])
    finally:
        dev.objective_grad_end()
    for name in DENSE if dense else TRELLIS:   # ... and the call is served once the evaluation has ended
        assert _call(dev, name, w) == (0, "")


def test_matrix_file_mode(monkeypatch):
    dev = _device(monkeypatch, True)
    dev.load_paths(2, [0, 1, 2], [0, 1], [1.0, 1.0], [0, 2], [0, 1], [1.0])
    for name in TRELLIS + DENSE:
        assert _call(dev, name, np.zeros(2)) == (ARG, MATRIX[name])


@pytest.mark.parametrize("dense", [True, False])
def test_arguments_then_tier_then_weights(dense, monkeypatch):
    """on each tier: a refused argument speaks before the wrong tier, the wrong
    tier before null or NaN weights, null weights before anything is touched"""
    w = _case()[4]
    dev = _device(monkeypatch, dense)
    nan = w.copy()
    nan[len(w) // 2] = np.nan
    for name in TRELLIS + DENSE:
        for bad, msg in BAD_ARG.get(name, []):
            assert _call(dev, name, w, **bad) == (ARG, msg)       # on its own tier and on the other
        if (name in DENSE) == dense:
            assert _call(dev, name, None) == (ARG, "null weights")
        else:
            assert _call(dev, name, w) == WRONG_TIER[name]
            assert _call(dev, name, nan) == WRONG_TIER[name]
            assert _call(dev, name, None) == WRONG_TIER[name]


def test_dense_weights_nan_and_plus_inf_refused_minus_inf_taken(monkeypatch):
    w = _case()[4]
    dev = _device(monkeypatch, True)
    for name in DENSE:
        for bad in (np.nan, np.inf):
            wb = w.copy()
            wb[len(w) // 2] = bad
            assert _call(dev, name, wb) == (ARG, NAN[name])
        wb = w.copy()
        wb[len(w) // 2] = -np.inf
        assert _call(dev, name, wb) == (0, "")
        for bad, msg in BAD_ARG.get(name, []):   # the argument speaks before the NaN
            wb[0] = np.nan
            assert _call(dev, name, wb, **bad) == (ARG, msg)


def test_a_refused_call_leaves_the_held_result(monkeypatch):
    """dense_sample_paths: a valid result, then a call with n = 0: _get still
    hands out the earlier result"""
    w = _case()[4]
    dev = _device(monkeypatch, True)
    srow, logw, prow, pidx, _ = dev.dense_sample_paths(w, 2, seed=7)
    assert len(logw) > 0 and len(pidx) > 0
    assert _call(dev, "dense_sample_paths", w, n=0) == (ARG, "dense_sample_paths: n = 0 is outside 1 .. 64")
    got = [np.zeros_like(a) for a in (srow, logw, prow, pidx)]
    assert _lib().wfsa_dev_dense_sample_paths_get(dev._h, *[a.ctypes.data for a in got]) == 0
    for a, b in zip(got, (srow, logw, prow, pidx)):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("dense", [True, False])
def test_getters_without_a_result(dense, monkeypatch):
    """all ten before any result, the tier's own after a result and a
    load_corpus, and what the byte-marginal getters say about a part that the
    last call did not ask for"""
    fsa, sym, off, p, w = _case()
    dev = _device(monkeypatch, dense)
    for getter in GETTERS:
        assert _get(dev, getter) == (ARG, NO_RESULT[getter])
    own = [g for g in GETTERS if g.startswith("dense_") == dense]
    for name in DENSE if dense else TRELLIS:
        assert _call(dev, name, w) == (0, "")
    for getter in own:
        assert _get(dev, getter) == (0, "")
    if dense:
        assert _call(dev, "dense_byte_marginals", w, rows=1, decode=0) == (0, "")
        assert _get(dev, "dense_byte_marginals_get") == (0, "")
        assert _get(dev, "dense_byte_marginals_path_get") == (
            ARG, "dense_byte_marginals_path_get: the last wfsa_dev_dense_byte_marginals call had decode = 0")
        assert _call(dev, "dense_byte_marginals", w, rows=0, decode=1) == (0, "")
        assert _get(dev, "dense_byte_marginals_path_get") == (0, "")
        assert _get(dev, "dense_byte_marginals_get") == (
            ARG, "dense_byte_marginals_get: the last wfsa_dev_dense_byte_marginals call had rows = 0")
    else:
        assert _call(dev, "byte_marginals", w, decode=0) == (0, "")
        assert _get(dev, "byte_marginals_get") == (0, "")
        assert _get(dev, "byte_marginals_path_get") == (ARG, "byte_marginals_path_get: the last wfsa_dev_byte_marginals call had decode = 0")
    dev.load_corpus(sym, off, p)
    for getter in GETTERS:
        assert _get(dev, getter) == (ARG, NO_RESULT[getter])


def test_getters_on_a_null_context():
    lib = _lib()
    for getter, n_out in GETTERS.items():
        assert getattr(lib, "wfsa_dev_" + getter)(None, *([None] * n_out)) == ARG
        assert lib.wfsa_dev_last_error().decode() == "null context"
