"""GPU tests of posterior path sampling (wfsa_dev_sample_paths, sample.hip): n
random accepting paths per string from P(path | string) = exp(w(path)) / q_s,
against the oracle's enumerated paths (decode_cases: P, mrow) and the numpy
restatement of the generator (sample_reference.py).

Every sample must be a path of its string with the weight the oracle gives it
(decode_cases._tol, the decode tolerance); log q must match the log-sum-exp of
the enumerated weights within 1e-11 max(1, |log q|), also where
q_s lies below the double range; the draws must fit the exact posterior by the
chi-square condition test_sample_reference.py shows to be fair and to have
power; a posterior sharper than 2^-53 must always give the Viterbi path, byte
for byte; samples of strings with at most 16 paths must be k-best entries,
byte for byte; and the reproducibility contract of include/wfsa_dev.h holds.
Needs a gfx950 device."""
import ctypes as C
import functools

import numpy as np
import pytest

import sample_reference as R
from decode_cases import GOLDEN, _big, _device, _family, _golden, _reference, _source, _tol

pytestmark = pytest.mark.gpu

CASES = [c[0] for c in GOLDEN] + ["amb12", "compiled64", "wide200", "long64"]


def _weights(ref, dev, rng, mean=-1.0):
    """a random trimmed x (drawn as the decode tests draw it) and the device's w_full for it"""
    o = ref["o"]
    x = rng.normal(mean, 0.5, size=o.n)
    o.set_x(x)
    return x, o.w_full()[dev.perm]


@functools.lru_cache(maxsize=None)
def _many():
    """compiled64's shape with more strings than waves can be in flight (256 CUs x 16)"""
    import wfsa_amd as W
    syn = W.Synthetic(n_states=64, degree=4, vocab=16, emissions=1, n_strings=9000, max_len=10, seed=3)
    sym, off, wt = syn.corpus()
    return _reference(syn.wfsa_text, sym, off, wt)


def _ref_of(name):
    return _many() if name == "many9000" else _source(name)


@functools.lru_cache(maxsize=None)
def _tables(name):
    """a 64-bit hash per oracle path that its count row determines (a sum of
    per-parameter random words, wrapping), and per recognized string the map
    hash -> first path with that row: a sample's row is looked up by hash and
    then compared exactly"""
    ref = _ref_of(name)
    P, mrow = ref["P"], ref["mrow"]
    h = np.random.default_rng(1).integers(1, 2 ** 63, size=P.shape[1], dtype=np.uint64)
    hp = (P.astype(np.uint64) * h[None, :]).sum(axis=1, dtype=np.uint64)
    first = []
    for r in range(len(mrow) - 1):
        m = {}
        for l in range(mrow[r], mrow[r + 1]):
            m.setdefault(int(hp[l]), l)
        first.append(m)
    return h, first


def _sample_hashes(ref, h, perm, prow, pidx):
    """the hash of every returned path's count row; no id may be a trimmed-away parameter"""
    tr = ref["trim"][perm[pidx]]
    assert (tr != -2).all()   # no unused parameter lies on a path
    hv = np.where(tr >= 0, h[np.maximum(tr, 0)], np.uint64(0)).astype(np.uint64)
    cs = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(hv, dtype=np.uint64)])
    return cs[prow[1:]] - cs[prow[:-1]], tr


def _accept(name, ref, x, perm, w_dev, n, result, strings):
    """item 2: every recognized string with a finite path owns exactly n paths,
    each the ids of an oracle path of that string with its weight"""
    srow, logw, prow, pidx, logq = result
    P, mrow = ref["P"], ref["mrow"]
    h, first = _tables(name)
    lw = R.path_weights(P, x)
    assert len(strings) == len(mrow) - 1
    assert srow[0] == 0 and srow[-1] == len(logw) and len(prow) == len(logw) + 1
    assert prow[0] == 0 and prow[-1] == len(pidx) and (np.diff(prow) >= 0).all()
    hs, tr = _sample_hashes(ref, h, perm, prow, pidx)
    for r, s in enumerate(strings):
        a, b = mrow[r], mrow[r + 1]
        want = n if np.isfinite(lw[a:b]).any() else 0
        assert srow[s + 1] - srow[s] == want, (s, srow[s + 1] - srow[s], want)
        for t in range(srow[s], srow[s + 1]):
            ids = pidx[prow[t]:prow[t + 1]]
            tol = _tol(logw[t])
            assert abs(w_dev[ids].sum() - logw[t]) <= tol, (s, t, w_dev[ids].sum(), logw[t])
            l = first[r].get(int(hs[t]))
            assert l is not None, (s, t, ids)   # the row of SOME oracle path of this string
            tt = tr[prow[t]:prow[t + 1]]
            assert (np.bincount(tt[tt >= 0], minlength=P.shape[1]) == P[l]).all(), (s, t, ids)
            assert abs(lw[l] - logw[t]) <= tol, (s, t, lw[l], logw[t])


def _logq_check(ref, x, logq, strings):
    """item 3: log q against the log-sum-exp of the oracle's enumerated path weights"""
    mrow = ref["mrow"]
    lw = R.path_weights(ref["P"], x)
    worst = 0.0
    for r, s in enumerate(strings):
        want = R.logsumexp(lw[mrow[r]:mrow[r + 1]])
        if not np.isfinite(want):
            assert logq[s] == -np.inf, (s, logq[s])
            continue
        err = abs(logq[s] - want) / max(1.0, abs(want))
        worst = max(worst, err)
        assert err <= 1e-11, (s, logq[s], want)
    return worst


@pytest.mark.parametrize("n", [1, 5, 64])
@pytest.mark.parametrize("name", CASES)
def test_every_sample_is_a_path(name, n, monkeypatch):
    """three weight draws; wide200 has more than 64 destinations per byte (several lane rounds)"""
    ref = _source(name)
    dev = _device(ref, monkeypatch)
    if name == "wide200":
        assert dev.stats()["n_nodes"] > 64
    rng = np.random.default_rng(5)
    n_all = len(ref["off"]) - 1
    miss = np.setdiff1d(np.arange(n_all), ref["rec"])
    for draw in range(3):
        x, w = _weights(ref, dev, rng)
        result = dev.sample_paths(w, n, seed=draw)
        assert result[0].shape == (n_all + 1,) and result[4].shape == (n_all,)
        _accept(name, ref, x, dev.perm, w, n, result, ref["rec"])
        _logq_check(ref, x, result[4], ref["rec"])
        assert np.all(np.diff(result[0])[miss] == 0) and np.all(result[4][miss] == -np.inf)   # unrecognized: no sample
    assert dev.stats()["sample_path_ms"] > 0.0


@pytest.mark.parametrize("tier2", [False, True], ids=["tier2=0", "tier2=1"])
@pytest.mark.parametrize("name", ["test3", "amb12"])
def test_whichever_tier_serves_the_learning_path(name, tier2, monkeypatch):
    ref = _source(name)
    dev = _device(ref, monkeypatch, tier2=tier2)
    if tier2:
        dev.recognize()
    x, w = _weights(ref, dev, np.random.default_rng(17))
    result = dev.sample_paths(w, 5, seed=1)
    _accept(name, ref, x, dev.perm, w, 5, result, ref["rec"])
    other = _device(ref, monkeypatch, tier2=not tier2).sample_paths(w, 5, seed=1)
    for u, v in zip(result, other):
        assert u.tobytes() == v.tobytes()


@pytest.mark.parametrize("name", ["amb12", "compiled64", "wide200", "long64"])
def test_logq_agrees_with_the_evaluation(name, monkeypatch):
    """log q from the sampler's forward pass and from objective_grad on the same device"""
    ref = _family(name)
    dev = _device(ref, monkeypatch)
    x, w = _weights(ref, dev, np.random.default_rng(29))
    logq = dev.sample_paths(w, 1)[4]
    print(name, "worst relative log q error against the oracle:", _logq_check(ref, x, logq, ref["rec"]))
    _, _, elogq = dev.objective_grad(w, want_logq=True)
    err = np.abs(logq - elogq) / np.maximum(1.0, np.abs(elogq))
    print(name, "against objective_grad:", err.max())
    assert (err <= 1e-11).all()


def test_deep_weights_keep_their_samples(monkeypatch):
    """long64 at x ~ N(-12, 0.5): q_s of the long strings lies below the double
    range (log q < -745); the rescaled rows still give n valid samples and log q"""
    ref = _family("long64")
    dev = _device(ref, monkeypatch)
    x, w = _weights(ref, dev, np.random.default_rng(37), mean=-12.0)
    lw = R.path_weights(ref["P"], x)
    mrow = ref["mrow"]
    want = np.array([R.logsumexp(lw[mrow[r]:mrow[r + 1]]) for r in range(len(mrow) - 1)])
    deep = np.flatnonzero(want < -745.0)
    assert len(deep) > 0 and np.isfinite(want).all()
    result = dev.sample_paths(w, 64, seed=3)
    _accept("long64", ref, x, dev.perm, w, 64, result, ref["rec"])
    _logq_check(ref, x, result[4], ref["rec"])
    assert (np.diff(result[0])[ref["rec"][deep]] == 64).all()
    assert (result[4][ref["rec"][deep]] < -745.0).all()


@pytest.mark.parametrize("name", R.DIST_CASES)
def test_samples_follow_the_posterior(name, monkeypatch):
    """64 samples x 16 seeds per string against the exact posterior over the
    string's distinct count rows: X^2 <= dof + 6 sqrt(2 dof) (a condition: mean
    dof, standard deviation sqrt(2 dof); test_sample_reference.py shows that
    uniform draws and draws at other weights fail it)"""
    ref = _family(name)
    dev = _device(ref, monkeypatch)
    x, w = R.dist_weights(ref, dev.perm)
    cells = R.posterior_cells(ref, x)
    h, first = _tables(name)
    mrow, P = ref["mrow"], ref["P"]
    n_str = len(mrow) - 1
    assert (ref["rec"] == np.arange(n_str)).all()
    # path -> cell of its string
    cell_of = [{hv: cells[r][0][P[l].astype(np.int64).tobytes()] for hv, l in first[r].items()} for r in range(n_str)]
    counts = [np.zeros(len(c[1])) for c in cells]
    for seed in R.DIST_SEEDS:
        srow, logw, prow, pidx, _ = dev.sample_paths(w, R.DIST_N, seed=seed)
        assert (np.diff(srow) == R.DIST_N).all()
        hs, _ = _sample_hashes(ref, h, dev.perm, prow, pidx)
        for r in range(n_str):
            for t in range(srow[r], srow[r + 1]):
                counts[r][cell_of[r][int(hs[t])]] += 1   # (KeyError: not a row of this string)
    n = R.DIST_N * len(R.DIST_SEEDS)
    x2, dof, impossible = R.chi_square(cells, counts, n)
    print(name, "X^2", x2, "dof", dof, "bound", R.bound(dof))
    assert dof >= 200
    assert impossible == 0
    assert x2 <= R.bound(dof), (x2, dof)


def _same_as_best(dev, w, strings, n=64, seed=11):
    best, bprow, bpidx = dev.best_paths(w)
    srow, logw, prow, pidx, _ = dev.sample_paths(w, n, seed=seed)
    for s in strings:
        assert srow[s + 1] - srow[s] == n
        want_ids = bpidx[bprow[s]:bprow[s + 1]].tobytes()
        want_w = best[s:s + 1].tobytes()
        for t in range(srow[s], srow[s + 1]):
            assert pidx[prow[t]:prow[t + 1]].tobytes() == want_ids, (s, t)
            assert logw[t:t + 1].tobytes() == want_w, (s, t)


@pytest.mark.parametrize("name", ["amb12", "long64", "test3"])
def test_sharp_posteriors_give_the_viterbi_path(name, monkeypatch):
    """weights times 200: where the best path beats the second by more than 45
    in log weight (the rest of the posterior is below 2^-53 of it: paths times
    e^-45 < 2^-53, asserted), all 64 samples are best_paths' path, byte for byte"""
    ref = _source(name)
    dev = _device(ref, monkeypatch)
    x, w = _weights(ref, dev, np.random.default_rng(41))
    x, w = 200.0 * x, 200.0 * w
    lw = R.path_weights(ref["P"], x)
    mrow = ref["mrow"]
    sharp, most = [], 0
    for r in range(len(mrow) - 1):
        v = np.sort(lw[mrow[r]:mrow[r + 1]])[::-1]
        if len(v) >= 2 and v[0] - v[1] > 45.0:
            sharp.append(ref["rec"][r])
            most = max(most, len(v))
    assert len(sharp) > 0
    assert most * np.exp(-45.0) < 2.0 ** -53
    _same_as_best(dev, w, sharp)


def test_single_path_strings_give_that_path(monkeypatch):
    ref = _family("compiled64")
    dev = _device(ref, monkeypatch)
    _, w = _weights(ref, dev, np.random.default_rng(43))
    single = ref["rec"][np.flatnonzero(np.diff(ref["mrow"]) == 1)]
    assert len(single) > 0
    _same_as_best(dev, w, single)


@pytest.mark.parametrize("name", ["compiled64", "test3", "test5"])
def test_samples_are_kbest_entries(name, monkeypatch):
    """strings with at most 16 finite paths: every sample's ids and weight are
    byte-equal to one of the string's kbest_paths(w, 16) entries"""
    ref = _source(name)
    dev = _device(ref, monkeypatch)
    _, w = _weights(ref, dev, np.random.default_rng(47))
    n_paths = np.diff(ref["mrow"])
    few = ref["rec"][np.flatnonzero(n_paths <= 16)]
    assert len(few) > 0 and (name == "test5" or (n_paths[n_paths <= 16] > 1).any())
    ks, kl, kp, ki = dev.kbest_paths(w, 16)
    srow, logw, prow, pidx, _ = dev.sample_paths(w, 64, seed=5)
    for s in few:
        entries = {(ki[kp[t]:kp[t + 1]].tobytes(), kl[t:t + 1].tobytes()) for t in range(ks[s], ks[s + 1])}
        assert srow[s + 1] - srow[s] == 64
        for t in range(srow[s], srow[s + 1]):
            assert (pidx[prow[t]:prow[t + 1]].tobytes(), logw[t:t + 1].tobytes()) in entries, (s, t)


def test_sample_paths_with_minus_infinity_weights(monkeypatch):
    """the most-used quarter of amb12_seed7's used parameters at -inf (as the
    K-best test builds it): strings without a finite path own no sample and
    report log q = -inf, no sample carries a -inf parameter"""
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
    lw = R.path_weights(P, x)
    assert not np.isnan(lw).any()
    finite = np.array([np.isfinite(lw[mrow[r]:mrow[r + 1]]).sum() for r in range(len(mrow) - 1)])
    assert (finite >= 1).any() and ((finite == 0) & (np.diff(mrow) > 0)).any()
    result = dev.sample_paths(w, 64, seed=2)
    srow, logw, prow, pidx, logq = result
    _accept("amb12_seed7", ref, x, dev.perm, w, 64, result, ref["rec"])
    _logq_check(ref, x, logq, ref["rec"])
    none = ref["rec"][finite == 0]
    assert (np.diff(srow)[none] == 0).all() and (logq[none] == -np.inf).all()
    assert np.isfinite(w[pidx]).all()
    assert np.isfinite(logw).all() and np.isfinite(logq[ref["rec"][finite > 0]]).all()


def test_reproducibility_contract(monkeypatch):
    ref = _family("long64")
    dev = _device(ref, monkeypatch)
    _, w = _weights(ref, dev, np.random.default_rng(3))
    first = dev.sample_paths(w, 64, seed=9)
    second = dev.sample_paths(w, 64, seed=9)
    for u, v in zip(first, second):
        assert u.tobytes() == v.tobytes()
    # the first 5 of the n = 64 result are the n = 5 result
    s64, l64, p64, i64, q64 = first
    s5, l5, p5, i5, q5 = dev.sample_paths(w, 5, seed=9)
    assert q5.tobytes() == q64.tobytes()
    assert (np.diff(s5) == 5).all() and (np.diff(s64) == 64).all()
    for s in range(len(s5) - 1):
        assert l64[s64[s]:s64[s] + 5].tobytes() == l5[s5[s]:s5[s + 1]].tobytes()
        assert i64[p64[s64[s]]:p64[s64[s] + 5]].tobytes() == i5[p5[s5[s]]:p5[s5[s + 1]]].tobytes()
        assert (p64[s64[s]:s64[s] + 6] - p64[s64[s]]).tobytes() == (p5[s5[s]:s5[s + 1] + 1] - p5[s5[s]]).tobytes()
    # another seed continues the sample set with other draws
    other = dev.sample_paths(w, 64, seed=10)
    assert other[4].tobytes() == q64.tobytes()
    assert other[3].tobytes() != i64.tobytes()


@pytest.mark.parametrize("seed,string,sample", [(0, 0, 0), (1, 2, 3), (0xDEADBEEFCAFEF00D, 7, 63), (5, (1 << 32) + 17, 1),
                                                ((1 << 63) + 12345, (3 << 32) | 0xFFFFFFFF, 40)])
def test_generator_is_the_stated_philox(seed, string, sample):
    import wfsa_amd as W
    got = W.sample_uniforms(seed, string, sample, 300)
    assert got.tobytes() == R.uniforms(seed, string, sample, 300).tobytes()
    assert ((got >= 0.0) & (got < 1.0)).all()


def test_more_strings_than_waves_in_flight(monkeypatch):
    """9,000 strings on at most 4,096 waves: the ticket and the rows' reset between strings"""
    ref = _many()
    dev = _device(ref, monkeypatch)
    n_all = len(ref["off"]) - 1
    assert n_all == 9000 and len(ref["rec"]) == 9000 and n_all > 16 * 256
    x, w = _weights(ref, dev, np.random.default_rng(53))
    result = dev.sample_paths(w, 5, seed=4)
    _accept("many9000", ref, x, dev.perm, w, 5, result, ref["rec"])
    _logq_check(ref, x, result[4], ref["rec"])


def test_sampler_leaves_the_quasinewton_loop_alone():
    """Run(3), Run(3) gives info rows bit-equal to Run(3), SamplePaths(8), Run(3) (rmin column on)"""
    import wfsa_amd as W
    fsa, sym, off, wt = _big()
    runs = []
    for sample in (False, True):
        lrn = W.QuasiNewtonLearner(0)
        lrn.set_info_rmin(True)
        lrn.BuildFromPacked(fsa, sym, off, wt)
        lrn.Finalize()
        lrn.Init(7)
        rows = lrn.Run(3, 1.0, -1.0)
        if sample:
            srow, logw, prow, pidx, logq = lrn.SamplePaths(8, seed=6)
            assert np.isfinite(logw).all() and (np.diff(srow) == 8).all() and (np.diff(prow) > 0).all()
            assert np.isfinite(logq).all() and (logw <= np.repeat(logq, 8) + 1e-9).all()
        rows += lrn.Run(3, 1.0, -1.0)
        runs.append(np.array(rows))
    assert runs[0].shape == (6, 7)
    assert runs[0].tobytes() == runs[1].tobytes()
    assert W.HessianLearner.SamplePaths is W.QuasiNewtonLearner.SamplePaths


def _get(fn, dev, like):
    out = [np.zeros_like(v) for v in like]
    assert fn(dev._h, *(v.ctypes.data_as(C.c_void_p) for v in out)) == 0
    return out


def test_sampler_leaves_rmin_and_the_decoders_alone():
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
    dev.sample_paths(w2, 8, seed=1)
    assert dev.rmin() == plain
    # the decoders' results outlive a sample_paths call ...
    _, bprow, bpidx = dev.best_paths(w1)
    kb = dev.kbest_paths(w1, 4)
    sp = dev.sample_paths(w2, 8, seed=1)
    for u, v in zip((bprow, bpidx), _get(lib.wfsa_dev_best_paths_get, dev, (bprow, bpidx))):
        assert u.tobytes() == v.tobytes()
    for u, v in zip(kb, _get(lib.wfsa_dev_kbest_paths_get, dev, kb)):
        assert u.tobytes() == v.tobytes()
    # ... and the other way round
    dev.best_paths(w2)
    dev.kbest_paths(w2, 4)
    for u, v in zip(sp[:4], _get(lib.wfsa_dev_sample_paths_get, dev, sp[:4])):
        assert u.tobytes() == v.tobytes()


def test_sample_paths_errors(monkeypatch):
    import wfsa_amd as W
    from wfsa_amd import _lib
    ref = _golden("talk", "talk")
    fsa = W.Fsa.read_text(ref["text"])
    # before a model and a corpus are loaded
    dev = W.Device(0)
    with pytest.raises(W.WfsaError) as e:
        dev.sample_paths(np.zeros(0), 4)
    assert e.value.code == _lib.WFSA_ERR_ARG
    dev.load_model(fsa)
    with pytest.raises(W.WfsaError) as e:
        dev.sample_paths(np.zeros(dev.n_params), 4)
    assert e.value.code == _lib.WFSA_ERR_ARG
    # _get without a result since the last load
    dev.load_corpus(ref["sym"], ref["off"], ref["wt"] / ref["wt"].sum())
    srow = np.zeros(dev.n_strings + 1, dtype=np.int64)
    assert W.load().wfsa_dev_sample_paths_get(dev._h, srow.ctypes.data_as(C.c_void_p), None, None, None) == _lib.WFSA_ERR_ARG
    # while an evaluation is in flight
    w = np.full(dev.n_params, -1.0)
    dev.objective_grad_begin(w)
    with pytest.raises(W.WfsaError) as e:
        dev.sample_paths(w, 4)
    assert e.value.code == _lib.WFSA_ERR_ARG and "in flight" in str(e.value)
    dev.objective_grad_end()
    # n outside 1 .. WFSA_SAMPLE_MAX
    for n in (0, 65):
        with pytest.raises(W.WfsaError) as e:
            dev.sample_paths(w, n)
        assert e.value.code == _lib.WFSA_ERR_ARG and "n = %d" % n in str(e.value)
    srow, logw, _, _, logq = dev.sample_paths(w, 64)
    assert (np.diff(srow) == 64).sum() == 3 and (np.diff(srow) == 0).sum() == 2 and np.isfinite(logw).all()
    assert np.isfinite(logq).sum() == 3
    assert W.load().wfsa_dev_sample_paths_get(dev._h, srow.ctypes.data_as(C.c_void_p), None, None, None) == 0
    # a load drops the result
    dev.load_corpus(ref["sym"], ref["off"], ref["wt"] / ref["wt"].sum())
    assert W.load().wfsa_dev_sample_paths_get(dev._h, srow.ctypes.data_as(C.c_void_p), None, None, None) == _lib.WFSA_ERR_ARG
    # matrix-file mode: no automaton
    dev.load_paths(2, [0, 1, 2], [0, 1], [1.0, 1.0], [0, 2], [0, 1], [1.0])
    with pytest.raises(W.WfsaError) as e:
        dev.sample_paths(np.zeros(2), 4)
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
        dd.sample_paths(np.full(dd.n_params, -1.0), 4)
    assert e.value.code == _lib.WFSA_ERR_CAPACITY and "WFSA_DENSE=0" in str(e.value)
