"""GPU tests of posterior expected counts (wfsa_dev_posterior_counts,
posterior.hip): per string log q, the entropy of its path posterior and the
sparse row of expected parameter counts, against the exact E-step from the
oracle's enumerated paths (posterior_reference.py over decode_cases: P, mrow).

log q must match the log-sum-exp of the enumerated weights within
1e-11 max(1, |log q|).  Counts and entropy are compared per string,
relative to max(1, value), under a cap that follows from that bound: a mass is
exp of a three-term difference of log alphas, chained over the string's L + 1
steps: 3e-11 max(1, |log q_s|) (L_s + 1).  The cap only stops a wrong kernel
from passing; the parity test prints the measured worst errors (committed in
profiles/posterior_counts/errors.json; measured worst: 1.6e-13 for a count,
9.0e-14 for an entropy, 8.9e-16 for log q).  Needs a gfx950 device."""
import ctypes as C

import numpy as np
import pytest

import posterior_reference as PR
import sample_reference as R
from decode_cases import GOLDEN, _big, _device, _family, _golden, _source
from test_gpu_sample_paths import _get, _many, _weights

pytestmark = pytest.mark.gpu

CASES = [c[0] for c in GOLDEN] + ["amb12", "compiled64", "wide200", "long64"]


def _check(ref, x, dev, w, result):
    """the result against the reference at x on the recognized strings: (worst
    count error, worst entropy error, worst log q error), each relative to
    max(1, value)"""
    crow, cidx, cval, logq, entropy = result
    n_all = len(ref["off"]) - 1
    rec = ref["rec"]
    assert crow.shape == (n_all + 1,) and logq.shape == (n_all,) and entropy.shape == (n_all,)
    assert crow[0] == 0 and crow[-1] == len(cidx) == len(cval) and (np.diff(crow) >= 0).all()
    assert (cval > 0.0).all() and not np.isnan(cval).any()
    for s in range(n_all):
        assert (np.diff(cidx[crow[s]:crow[s + 1]]) > 0).all(), s   # ascending ids
    want_lq, want_c, want_h = PR.posterior(ref, x)
    lengths = np.diff(ref["off"])[rec]
    got_c, listed = PR.device_rows(ref, dev.perm, crow, cidx, cval, rec)
    worst = [0.0, 0.0, 0.0]
    for r in range(len(rec)):
        s = rec[r]
        if not np.isfinite(want_lq[r]):   # no path of finite weight: nothing
            assert crow[s + 1] == crow[s] and logq[s] == -np.inf and np.isnan(entropy[s]), s
            continue
        assert crow[s + 1] > crow[s], s
        e_lq = abs(logq[s] - want_lq[r]) / max(1.0, abs(want_lq[r]))
        assert e_lq <= 1e-11, (s, logq[s], want_lq[r])
        cap = PR.cap(want_lq[r], lengths[r])
        e_c = (np.abs(got_c[r] - want_c[r]) / np.maximum(1.0, want_c[r])).max()
        assert e_c <= cap, (s, e_c, cap)
        assert entropy[s] >= 0.0
        e_h = abs(entropy[s] - want_h[r]) / max(1.0, want_h[r])
        assert e_h <= cap, (s, entropy[s], want_h[r], cap)
        assert listed[r][want_c[r] > 1e-9].all(), s       # every parameter used in expectation is listed
        assert (want_c[r][listed[r]] > 0.0).all(), s      # and nothing else
        worst = [max(worst[0], e_c), max(worst[1], e_h), max(worst[2], e_lq)]
    return worst


def _unrecognized_own_nothing(ref, result):
    crow, _, _, logq, entropy = result
    miss = np.setdiff1d(np.arange(len(ref["off"]) - 1), ref["rec"])
    assert (np.diff(crow)[miss] == 0).all() and (logq[miss] == -np.inf).all() and np.isnan(entropy[miss]).all()


@pytest.mark.parametrize("name", CASES)
def test_rows_entropy_and_logq_match_the_enumeration(name, monkeypatch):
    """three weight draws; wide200 has more than 64 destinations per byte
    (several lane rounds), long64 strings of 64 positions"""
    ref = _source(name)
    dev = _device(ref, monkeypatch)
    if name == "wide200":
        assert dev.stats()["n_nodes"] > 64
    rng = np.random.default_rng(5)
    worst = [0.0, 0.0, 0.0]
    for draw in range(3):
        x, w = _weights(ref, dev, rng)
        result = dev.posterior_counts(w)
        worst = [max(a, b) for a, b in zip(worst, _check(ref, x, dev, w, result))]
        _unrecognized_own_nothing(ref, result)
    print("posterior_counts errors", name, "count %.3e entropy %.3e logq %.3e" % tuple(worst))
    assert dev.stats()["posterior_count_ms"] > 0.0


def test_single_path_strings_are_exact(monkeypatch):
    """compiled64: every string with exactly one path reports that path's
    integer counts exactly and entropy exactly 0 (every mass is exp(0) = 1)"""
    ref = _family("compiled64")
    dev = _device(ref, monkeypatch)
    x, w = _weights(ref, dev, np.random.default_rng(41))
    result = dev.posterior_counts(w)
    crow, cidx, cval, logq, entropy = result
    P, mrow, rec = ref["P"], ref["mrow"], ref["rec"]
    single = np.flatnonzero(np.diff(mrow) == 1)
    assert len(single) >= 100
    got, _ = PR.device_rows(ref, dev.perm, crow, cidx, cval, rec)
    for r in single:
        assert (got[r] == P[mrow[r]]).all(), r
        assert entropy[rec[r]] == 0.0, (r, entropy[rec[r]])
        vals = cval[crow[rec[r]]:crow[rec[r] + 1]]
        assert (vals == np.rint(vals)).all()


@pytest.mark.parametrize("name", ["amb12", "long64"])
def test_logq_has_the_samplers_bits(name, monkeypatch):
    ref = _family(name)
    dev = _device(ref, monkeypatch)
    _, w = _weights(ref, dev, np.random.default_rng(43))
    logq = dev.posterior_counts(w)[3]
    assert logq.tobytes() == dev.sample_paths(w, 1)[4].tobytes()


def test_deep_weights_keep_their_rows(monkeypatch):
    """long64 at x ~ N(-12, 0.5), as the sampler's test builds it: q_s of the
    long strings lies below the double range (log q < -745); their rows and
    entropy stay within the cap and none is empty"""
    ref = _family("long64")
    dev = _device(ref, monkeypatch)
    x, w = _weights(ref, dev, np.random.default_rng(37), mean=-12.0)
    lw = R.path_weights(ref["P"], x)
    mrow = ref["mrow"]
    want = np.array([R.logsumexp(lw[mrow[r]:mrow[r + 1]]) for r in range(len(mrow) - 1)])
    deep = np.flatnonzero(want < -745.0)
    assert len(deep) > 0 and np.isfinite(want).all()
    result = dev.posterior_counts(w)
    print("posterior_counts errors long64_deep count %.3e entropy %.3e logq %.3e" % tuple(_check(ref, x, dev, w, result)))
    assert (np.diff(result[0])[ref["rec"][deep]] > 0).all()
    assert (result[3][ref["rec"][deep]] < -745.0).all()


def test_minus_infinity_weights(monkeypatch):
    """the most-used quarter of amb12_seed7's used parameters at -inf (as the
    sampler's test builds it): no listed id has a -inf weight, strings without
    a finite path own nothing, the rest agree with the reference without the
    -inf paths, and no NaN but the entropy of the strings of mass 0"""
    ref = _family("amb12_seed7")
    dev = _device(ref, monkeypatch)
    P, mrow, trim = ref["P"], ref["mrow"], ref["trim"]
    x, w = _weights(ref, dev, np.random.default_rng(13))
    use = P.sum(axis=0)
    used = np.flatnonzero(use > 0)
    off = used[np.argsort(-use[used], kind="stable")][:len(used) // 4]
    x = x.copy()
    x[off] = -np.inf
    w = w.copy()
    w[np.isin(trim[dev.perm], off)] = -np.inf
    finite = PR.path_count(ref, x)
    assert (finite >= 1).any() and ((finite == 0) & (np.diff(mrow) > 0)).any()
    result = dev.posterior_counts(w)
    crow, cidx, cval, logq, entropy = result
    print("posterior_counts errors amb12_seed7_minus_inf count %.3e entropy %.3e logq %.3e" % tuple(_check(ref, x, dev, w, result)))
    assert np.isfinite(w[cidx]).all()
    none = ref["rec"][finite == 0]
    some = ref["rec"][finite > 0]
    assert (np.diff(crow)[none] == 0).all() and (logq[none] == -np.inf).all() and np.isnan(entropy[none]).all()
    assert np.isfinite(logq[some]).all() and np.isfinite(entropy[some]).all() and (np.diff(crow)[some] > 0).all()
    assert np.isfinite(cval).all() and not np.isnan(logq).any()


def test_more_strings_than_waves_and_the_same_bytes_again(monkeypatch):
    """9,000 strings on at most 4,096 waves, against the reference; a second
    call hands the tickets to other waves and returns the same bytes (the adds
    arrive in another order), and so does a call on 64 waves"""
    ref = _many()
    dev = _device(ref, monkeypatch)
    n_all = len(ref["off"]) - 1
    assert n_all == 9000 and len(ref["rec"]) == 9000 and n_all > 16 * 256
    x, w = _weights(ref, dev, np.random.default_rng(53))
    first = dev.posterior_counts(w)
    print("posterior_counts errors many9000 count %.3e entropy %.3e logq %.3e" % tuple(_check(ref, x, dev, w, first)))
    second = dev.posterior_counts(w)
    monkeypatch.setenv("WFSA_POSTERIOR_WAVES", "64")
    third = dev.posterior_counts(w)
    for other in (second, third):
        for u, v in zip(first, other):
            assert u.tobytes() == v.tobytes()


@pytest.mark.parametrize("name", ["test3", "amb12"])
def test_whichever_tier_serves_the_learning_path(name, monkeypatch):
    ref = _source(name)
    results = []
    for tier2 in (False, True):
        dev = _device(ref, monkeypatch, tier2=tier2)
        if tier2:
            dev.recognize()
        x, w = _weights(ref, dev, np.random.default_rng(17))
        results.append(dev.posterior_counts(w))
    _check(ref, x, dev, w, results[1])
    for u, v in zip(*results):
        assert u.tobytes() == v.tobytes()


def test_posterior_counts_leave_the_quasinewton_loop_alone():
    """Run(3), Run(3) gives info rows bit-equal to Run(3), PosteriorCounts(), Run(3) (rmin column on)"""
    import wfsa_amd as W
    fsa, sym, off, wt = _big()
    runs = []
    for call in (False, True):
        lrn = W.QuasiNewtonLearner(0)
        lrn.set_info_rmin(True)
        lrn.BuildFromPacked(fsa, sym, off, wt)
        lrn.Finalize()
        lrn.Init(7)
        rows = lrn.Run(3, 1.0, -1.0)
        if call:
            crow, cidx, cval, logq, entropy = lrn.PosteriorCounts()
            assert np.isfinite(logq).all() and (entropy >= 0.0).all() and (np.diff(crow) > 0).all() and (cval > 0.0).all()
        rows += lrn.Run(3, 1.0, -1.0)
        runs.append(np.array(rows))
    assert runs[0].shape == (6, 7)
    assert runs[0].tobytes() == runs[1].tobytes()
    assert W.HessianLearner.PosteriorCounts is W.QuasiNewtonLearner.PosteriorCounts


def test_posterior_counts_leave_rmin_and_the_other_results_alone():
    import wfsa_amd as W
    lib = W.load()
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
    dev.posterior_counts(w2)
    assert dev.rmin() == plain
    # the decoders' and the sampler's results outlive a posterior_counts call ...
    _, bprow, bpidx = dev.best_paths(w1)
    kb = dev.kbest_paths(w1, 4)
    sp = dev.sample_paths(w1, 8, seed=1)
    pc = dev.posterior_counts(w2)
    for u, v in zip((bprow, bpidx), _get(lib.wfsa_dev_best_paths_get, dev, (bprow, bpidx))):
        assert u.tobytes() == v.tobytes()
    for u, v in zip(kb, _get(lib.wfsa_dev_kbest_paths_get, dev, kb)):
        assert u.tobytes() == v.tobytes()
    for u, v in zip(sp[:4], _get(lib.wfsa_dev_sample_paths_get, dev, sp[:4])):
        assert u.tobytes() == v.tobytes()
    # ... and the other way round
    dev.best_paths(w1)
    dev.kbest_paths(w1, 4)
    dev.sample_paths(w1, 8, seed=1)
    for u, v in zip(pc[:3], _get(lib.wfsa_dev_posterior_counts_get, dev, pc[:3])):
        assert u.tobytes() == v.tobytes()


def test_posterior_counts_errors(monkeypatch):
    import wfsa_amd as W
    from wfsa_amd import _lib
    ref = _golden("talk", "talk")
    fsa = W.Fsa.read_text(ref["text"])
    # before a model and a corpus are loaded
    dev = W.Device(0)
    with pytest.raises(W.WfsaError) as e:
        dev.posterior_counts(np.zeros(0))
    assert e.value.code == _lib.WFSA_ERR_ARG
    dev.load_model(fsa)
    with pytest.raises(W.WfsaError) as e:
        dev.posterior_counts(np.zeros(dev.n_params))
    assert e.value.code == _lib.WFSA_ERR_ARG
    # _get without a result since the last load
    dev.load_corpus(ref["sym"], ref["off"], ref["wt"] / ref["wt"].sum())
    crow = np.zeros(dev.n_strings + 1, dtype=np.int64)
    assert W.load().wfsa_dev_posterior_counts_get(dev._h, crow.ctypes.data_as(C.c_void_p), None, None) == _lib.WFSA_ERR_ARG
    # while an evaluation is in flight
    w = np.full(dev.n_params, -1.0)
    dev.objective_grad_begin(w)
    with pytest.raises(W.WfsaError) as e:
        dev.posterior_counts(w)
    assert e.value.code == _lib.WFSA_ERR_ARG and "in flight" in str(e.value)
    dev.objective_grad_end()
    crow, cidx, cval, logq, entropy = dev.posterior_counts(w)
    assert (np.diff(crow) > 0).sum() == 3 and (np.diff(crow) == 0).sum() == 2
    assert np.isfinite(logq).sum() == 3 and np.isnan(entropy).sum() == 2
    assert W.load().wfsa_dev_posterior_counts_get(dev._h, crow.ctypes.data_as(C.c_void_p), None, None) == 0
    # a load drops the result
    dev.load_corpus(ref["sym"], ref["off"], ref["wt"] / ref["wt"].sum())
    assert W.load().wfsa_dev_posterior_counts_get(dev._h, crow.ctypes.data_as(C.c_void_p), None, None) == _lib.WFSA_ERR_ARG
    # matrix-file mode: no automaton
    dev.load_paths(2, [0, 1, 2], [0, 1], [1.0, 1.0], [0, 2], [0, 1], [1.0])
    with pytest.raises(W.WfsaError) as e:
        dev.posterior_counts(np.zeros(2))
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
        dd.posterior_counts(np.full(dd.n_params, -1.0))
    assert e.value.code == _lib.WFSA_ERR_CAPACITY and "WFSA_DENSE=0" in str(e.value)
