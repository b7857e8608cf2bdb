"""GPU tests of the K-best decode (wfsa_dev_kbest_paths, decode.hip): the k
most probable accepting paths of every string from the device's top-k
(max, +) trellis pass, against the oracle's enumerated paths
(oracle/hessian.py: the path-count matrix P and the strings' path rows mrow).

Acceptance, for EVERY recognized string, with m = min(k, the string's oracle
paths of finite weight): it returns m paths; their log weights do not
increase; the i-th equals the i-th largest oracle path weight within
1e-12 max(1, |value|) (the project's decode tolerance; a path sums at most ~70
terms of size ~1); each path's ids dotted with w_full reproduce its weight,
none is a trimmed-away parameter, and their counts are the P row of SOME oracle
path of the string whose weight is within the tolerance of the returned one;
and no count row is returned more often than the oracle has paths with it.
Two exact properties on top: k = 1 is wfsa_dev_best_paths byte for byte, and
the first j paths of a k result are the j result byte for byte.
Needs a gfx950 device."""
import ctypes as C

import numpy as np
import pytest

from decode_cases import GOLDEN, _big, _device, _family, _golden, _source, _tol

pytestmark = pytest.mark.gpu

# the k of each family's group: a capacity (2, 4, 8, 16) and a k below one
FAMILY_K = [("amb12", 2), ("amb12", 5), ("amb12", 16), ("compiled64", 4), ("compiled64", 3),
            ("wide200", 4), ("wide200", 5), ("long64", 8), ("long64", 5)]


def _weights(ref, dev, rng):
    """a random trimmed x (drawn as the Viterbi tests draw it) and the device's w_full for it"""
    o = ref["o"]
    x = rng.normal(-1.0, 0.5, size=o.n)
    o.set_x(x)
    return x, o.w_full()[dev.perm]


def _path_weights(P, x):
    """the oracle weight of every path: x . P over the columns with a positive
    count only (a plain P @ x turns 0 * -inf into NaN)"""
    with np.errstate(invalid="ignore"):
        return np.where(P > 0, P * x, 0.0).sum(axis=1)


def _accept(ref, x, perm, w_dev, k, result, strings):
    """the acceptance rule, for every recognized string; strings[r] = the
    index in srow of the oracle's r-th recognized string"""
    srow, logw, prow, pidx = result
    P, mrow, trim = ref["P"], ref["mrow"], ref["trim"]
    lw = _path_weights(P, x)
    assert len(strings) == len(mrow) - 1
    assert srow[0] == 0 and srow[-1] == len(logw) and len(prow) == len(logw) + 1
    assert prow[0] == 0 and prow[-1] == len(pidx) and (np.diff(prow) >= 0).all()
    for r, s in enumerate(strings):
        a, b = mrow[r], mrow[r + 1]
        finite = np.sort(lw[a:b][np.isfinite(lw[a:b])])[::-1]
        m = min(k, len(finite))
        assert srow[s + 1] - srow[s] == m, (s, srow[s + 1] - srow[s], m)
        got = logw[srow[s]:srow[s + 1]]
        assert (np.diff(got) <= 0).all(), (s, got)
        returned = {}
        for i in range(m):
            t = srow[s] + i
            tol = _tol(finite[i])
            assert abs(got[i] - finite[i]) <= tol, (s, i, got[i], finite[i])
            ids = pidx[prow[t]:prow[t + 1]]
            assert abs(w_dev[ids].sum() - got[i]) <= tol, (s, i, w_dev[ids].sum(), got[i])
            tr = trim[perm[ids]]
            assert (tr != -2).all(), (s, i, ids)   # no unused parameter lies on a path
            row = np.bincount(tr[tr >= 0], minlength=P.shape[1])
            same = (P[a:b] == row).all(axis=1)
            assert (same & (np.abs(lw[a:b] - got[i]) <= _tol(got[i]))).any(), (s, i, ids)
            key = row.tobytes()
            returned[key] = returned.get(key, 0) + 1
            # two paths may share a row (or an id list): no more of a row than the oracle has
            assert returned[key] <= int(same.sum()), (s, i, ids)


def _check_device(ref, dev, k, seed):
    rng = np.random.default_rng(seed)
    n_all = len(ref["off"]) - 1
    miss = np.setdiff1d(np.arange(n_all), ref["rec"])
    for _ in range(3):
        x, w = _weights(ref, dev, rng)
        result = dev.kbest_paths(w, k)
        assert result[0].shape == (n_all + 1,)
        _accept(ref, x, dev.perm, w, k, result, ref["rec"])
        assert np.all(np.diff(result[0])[miss] == 0)   # unrecognized: no path


@pytest.mark.parametrize("k", [1, 3, 16])
@pytest.mark.parametrize("case", GOLDEN, ids=lambda c: c[0])
def test_kbest_paths_golden_cases(case, k, monkeypatch):
    """talk recognizes 3 of 5 strings, test3 4 of 7 (with exact ties and
    duplicate path rows); test5 repeats a parameter 9 times on a path; most
    strings have fewer than 16 paths"""
    ref = _golden(*case)
    n_all = len(ref["off"]) - 1
    if case[0] == "talk":
        assert (len(ref["rec"]), n_all) == (3, 5)
    if case[0] == "test3":
        assert (len(ref["rec"]), n_all) == (4, 7)
    _check_device(ref, _device(ref, monkeypatch), k, seed=5)


def _assert_family_shape(name, ref):
    """the family is what its cases rely on (the oracle's path counts)"""
    n = np.diff(ref["mrow"])
    if name == "amb12":
        assert n.sum() == 51242 and n.max() == 823
        assert (n >= 16).sum() * 2 >= len(n)   # the lists are really full
    if name == "compiled64":
        assert n.sum() == 657 and len(n) == 400   # most strings have fewer than 4
        assert (n == 1).any() and (n > 1).any()
    if name == "long64":
        assert np.diff(ref["off"]).max() == 64


@pytest.mark.parametrize("name,k", FAMILY_K)
def test_kbest_paths_synthetic(name, k, monkeypatch):
    ref = _family(name)
    assert len(ref["rec"]) == len(ref["off"]) - 1   # every string recognized
    _assert_family_shape(name, ref)
    _check_device(ref, _device(ref, monkeypatch), k, seed=7)


def test_kbest_paths_with_minus_infinity_weights(monkeypatch):
    """the most-used quarter of amb12's used parameters at -inf: paths through
    them drop out of the lists, strings keep fewer than 16 paths or none"""
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
    lw = _path_weights(P, x)
    assert not np.isnan(lw).any()
    finite = np.array([np.isfinite(lw[mrow[r]:mrow[r + 1]]).sum() for r in range(len(mrow) - 1)])
    assert ((finite >= 1) & (finite <= 15)).any()
    assert ((finite == 0) & (np.diff(mrow) > 0)).any()
    result = dev.kbest_paths(w, 16)
    _accept(ref, x, dev.perm, w, 16, result, ref["rec"])
    assert np.isfinite(result[1]).all()


@pytest.mark.parametrize("tier2", [False, True], ids=["tier2=0", "tier2=1"])
@pytest.mark.parametrize("name", [c[0] for c in GOLDEN] + ["amb12", "compiled64", "wide200", "long64"])
def test_k1_is_the_viterbi_decode(name, tier2, monkeypatch):
    """kbest_paths(w, 1) and best_paths(w) give the same bytes, whichever tier
    serves the strings in the learning path"""
    ref = _source(name)
    dev = _device(ref, monkeypatch, tier2=tier2)
    if tier2:
        dev.recognize()
    _, w = _weights(ref, dev, np.random.default_rng(17))
    best, bprow, bpidx = dev.best_paths(w)
    srow, logw, prow, pidx = dev.kbest_paths(w, 1)
    has = np.isfinite(best)
    assert has.sum() == len(ref["rec"])
    assert srow.tobytes() == np.concatenate([[0], np.cumsum(has)]).astype(np.int64).tobytes()
    assert logw.tobytes() == best[has].tobytes()
    assert prow[srow].tobytes() == bprow.tobytes()
    assert pidx.tobytes() == bpidx.tobytes()


@pytest.mark.parametrize("name", ["amb12", "long64"])
def test_first_three_of_eight_are_the_three_best(name, monkeypatch):
    ref = _family(name)
    dev = _device(ref, monkeypatch)
    _, w = _weights(ref, dev, np.random.default_rng(19))
    s8, l8, p8, i8 = dev.kbest_paths(w, 8)
    s3, l3, p3, i3 = dev.kbest_paths(w, 3)
    n8, n3 = np.diff(s8), np.diff(s3)
    assert (n3 == np.minimum(n8, 3)).all() and (n8 > 3).any()
    for s in range(len(n3)):
        assert l8[s8[s]:s8[s] + n3[s]].tobytes() == l3[s3[s]:s3[s + 1]].tobytes()
        for j in range(n3[s]):
            t8, t3 = s8[s] + j, s3[s] + j
            assert i8[p8[t8]:p8[t8 + 1]].tobytes() == i3[p3[t3]:p3[t3 + 1]].tobytes()


def test_kbest_paths_repeat_byte_for_byte(monkeypatch):
    ref = _family("long64")
    dev = _device(ref, monkeypatch)
    _, w = _weights(ref, dev, np.random.default_rng(3))
    first = dev.kbest_paths(w, 8)
    second = dev.kbest_paths(w, 8)
    for u, v in zip(first, second):
        assert u.tobytes() == v.tobytes()
    assert dev.stats()["kbest_path_ms"] > 0.0


def test_kbest_decoder_leaves_the_quasinewton_loop_alone():
    """Run(3), Run(3) gives info rows bit-equal to Run(3), KBestPaths(4), Run(3)
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
            srow, logw, prow, pidx = lrn.KBestPaths(4)
            assert np.isfinite(logw).all() and (np.diff(srow) >= 1).all() and (np.diff(prow) > 0).all()
        rows += lrn.Run(3, 1.0, -1.0)
        runs.append(np.array(rows))
    assert runs[0].shape == (6, 7)
    assert runs[0].tobytes() == runs[1].tobytes()


def test_kbest_decoder_leaves_rmin_and_best_paths_alone():
    """rmin() after objective_grad, kbest_paths(other weights) equals rmin()
    without the interleaved call; a best_paths result fetched after a
    kbest_paths call is the one fetched before it"""
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
    dev.kbest_paths(w2, 4)
    assert dev.rmin() == plain
    _, prow, pidx = dev.best_paths(w1)
    kb = dev.kbest_paths(w2, 4)
    prow2, pidx2 = np.zeros_like(prow), np.zeros_like(pidx)
    rc = W.load().wfsa_dev_best_paths_get(dev._h, prow2.ctypes.data_as(C.c_void_p), pidx2.ctypes.data_as(C.c_void_p))
    assert rc == 0
    assert prow2.tobytes() == prow.tobytes() and pidx2.tobytes() == pidx.tobytes()
    # ... and the kbest_paths result outlives a best_paths call
    dev.best_paths(w1)
    n = len(kb[1])
    srow2, logw2, kprow2, kpidx2 = np.zeros_like(kb[0]), np.zeros(n), np.zeros(n + 1, dtype=np.int64), np.zeros_like(kb[3])
    rc = W.load().wfsa_dev_kbest_paths_get(dev._h, *(v.ctypes.data_as(C.c_void_p) for v in (srow2, logw2, kprow2, kpidx2)))
    assert rc == 0
    for u, v in zip(kb, (srow2, logw2, kprow2, kpidx2)):
        assert u.tobytes() == v.tobytes()


@pytest.mark.parametrize("source", ["test3", "amb12"])
def test_learner_kbest_paths_after_a_device_run(source):
    """QuasiNewtonLearner.KBestPaths(4) after run(flags=7, epochs=4) decodes at
    the state the device-resident loop left: the oracle at o.x() after the
    same four qn_steps"""
    import wfsa_amd as W
    ref = _source(source)
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
    result = lrn.KBestPaths(4)
    n_local = lrn.info()["n_local_strings"]
    assert result[0].shape == (n_local + 1,) and n_local == len(ref["rec"])
    _accept(ref, x, perm, w_dev, 4, result, np.arange(n_local))
    # HessianLearner inherits the method
    assert W.HessianLearner.KBestPaths is W.QuasiNewtonLearner.KBestPaths


def test_kbest_paths_errors(monkeypatch):
    import wfsa_amd as W
    from wfsa_amd import _lib
    ref = _golden("talk", "talk")
    fsa = W.Fsa.read_text(ref["text"])
    # before a corpus is loaded
    dev = W.Device(0)
    with pytest.raises(W.WfsaError) as e:
        dev.kbest_paths(np.zeros(0), 4)
    assert e.value.code == _lib.WFSA_ERR_ARG
    dev.load_model(fsa)
    with pytest.raises(W.WfsaError) as e:
        dev.kbest_paths(np.zeros(dev.n_params), 4)
    assert e.value.code == _lib.WFSA_ERR_ARG
    # while an evaluation is in flight
    dev.load_corpus(ref["sym"], ref["off"], ref["wt"] / ref["wt"].sum())
    w = np.full(dev.n_params, -1.0)
    dev.objective_grad_begin(w)
    with pytest.raises(W.WfsaError) as e:
        dev.kbest_paths(w, 4)
    assert e.value.code == _lib.WFSA_ERR_ARG and "in flight" in str(e.value)
    dev.objective_grad_end()
    # k outside 1 .. WFSA_KBEST_MAX
    for k in (0, 17):
        with pytest.raises(W.WfsaError) as e:
            dev.kbest_paths(w, k)
        assert e.value.code == _lib.WFSA_ERR_ARG and "k = %d" % k in str(e.value)
    srow, logw, _, _ = dev.kbest_paths(w, 16)
    assert (np.diff(srow) > 0).sum() == 3 and np.isfinite(logw).all()
    # matrix-file mode: no automaton
    dev.load_paths(2, [0, 1, 2], [0, 1], [1.0, 1.0], [0, 2], [0, 1], [1.0])
    with pytest.raises(W.WfsaError) as e:
        dev.kbest_paths(np.zeros(2), 4)
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
        dd.kbest_paths(np.full(dd.n_params, -1.0), 4)
    assert e.value.code == _lib.WFSA_ERR_CAPACITY and "WFSA_DENSE=0" in str(e.value)
