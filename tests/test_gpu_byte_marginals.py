"""GPU tests of the per-byte state posteriors and the max-expected-accuracy
decode (wfsa_dev_byte_marginals, marginals.hip) against a plain enumeration of
every string's accepting paths (marginal_reference.py).

log q must match the log-sum-exp of the enumerated weights within
1e-11 max(1, |log q|) and carry posterior_counts' bytes.  Masses and
boundaries are at most 1 and come from §3j's arithmetic, so the project's derived
cap applies (posterior_reference.cap: 3e-11 max(1, |log q_s|) (L_s + 1)); a score
is a sum of L_s masses: L_s times that cap.  The cap only stops a wrong kernel
from passing; the parity test prints the measured worst errors (committed in
profiles/byte_marginals/errors.json).  Needs a gfx950 device."""
import ctypes as C
import functools

import numpy as np
import pytest

import marginal_reference as MR
import posterior_reference as PR
from decode_cases import GOLDEN, _big, _device, _family, _golden, _source, _tol
from test_gpu_sample_paths import _get, _many, _ref_of, _weights

pytestmark = pytest.mark.gpu

CASES = [c[0] for c in GOLDEN] + ["amb12", "compiled64", "wide200", "long64"]

# (a) the string xy has three paths, ^ -> A1(x) -> A2(y) -> $, ^ -> B1(x) -> C2(y) -> $ and
# ^ -> B1(x) -> D2(y) -> $, of posterior 0.40, 0.35 and 0.25 at FIXTURE_A_WEIGHTS: the most
# probable path is A's, the analysis with the most bytes right in expectation is B1 - C2
FIXTURE_A = """
^
$
^  0
^ A1 0 B1 0
A1 x 0
A1 A2 0
A2 y 0
A2 $ 0
B1 x 0
B1 C2 0 D2 0
C2 y 0
C2 $ 0
D2 y 0
D2 $ 0
"""
FIXTURE_A_WEIGHTS = {("^", "T", "A1"): np.log(0.4), ("^", "T", "B1"): np.log(0.6),
                     ("B1", "T", "C2"): np.log(0.35 / 0.6), ("B1", "T", "D2"): np.log(0.25 / 0.6)}
# (b) one state that emits only xy
FIXTURE_B = """
^
$
^  0
^ X 0
X xy 0
X $ 0
"""


def fixture_device(text, word=b"xy", named=None):
    """a device holding the one string `word` under the fixture, its Fsa and w_full (0 but for `named`)"""
    import wfsa_amd as W
    fsa = W.Fsa.read_text(text)
    dev = W.Device(0)
    dev.load_model(fsa)
    dev.load_corpus(np.frombuffer(word, dtype=np.uint8), np.array([0, len(word)], dtype=np.int64), np.ones(1))
    return dev, fsa, fixture_weights(fsa, named)


def fixture_weights(fsa, named=None):
    named = named or {}
    names = fsa.param_names()
    assert set(named) <= set(names), (sorted(named), names)
    return np.array([named.get(n, 0.0) for n in names], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def _enum(name):
    """the enumeration of a case's whole corpus, in the device's numbering: built once, left unchanged"""
    import wfsa_amd as W
    ref = _ref_of(name)
    return MR.enumerate_corpus(W.Fsa.read_text(ref["text"]), ref["sym"], ref["off"])


def _match(entry, ids):
    """the enumerated paths of a string whose parameter list is `ids`"""
    ids = [int(v) for v in ids]
    return [l for l, p in enumerate(entry["params"]) if p == ids]


def _check(ref, en, w, result, kbest=None):
    """a result (with or without the decode) against the enumeration at w_full on
    every string: (worst mass error, worst boundary error, worst log q error
    relative to max(1, |log q|), worst score error in units of L x cap)"""
    decode = len(result) == 9
    mrow, midx, mval, boundary, logq = result[:5]
    off = ref["off"]
    n_all, total = len(off) - 1, int(off[-1])
    n_states = en["n_states"]
    assert mrow.shape == (total + 1,) and boundary.shape == (total,) and logq.shape == (n_all,)
    assert mrow[0] == 0 and mrow[-1] == len(midx) == len(mval) and (np.diff(mrow) >= 0).all()
    assert (mval > 0.0).all() and (mval <= 1.0).all() and not np.isnan(logq).any()
    assert ((midx >= 0) & (midx < n_states)).all()
    if decode:
        score, plw, prow, pidx = result[5:]
        assert score.shape == plw.shape == (n_all,) and prow.shape == (n_all + 1,)
        assert prow[0] == 0 and prow[-1] == len(pidx) and (np.diff(prow) >= 0).all()
    worst = [0.0, 0.0, 0.0, 0.0]
    for s in range(n_all):
        entry = en["strings"][s]
        L = entry["L"]
        want = MR.derive(entry, w, n_states)
        b0 = int(off[s])
        if not np.isfinite(want["logq"]):   # no path of finite weight: nothing
            assert logq[s] == -np.inf and mrow[b0 + L] == mrow[b0] and np.isnan(boundary[b0:b0 + L]).all(), s
            if decode:
                assert np.isnan(score[s]) and plw[s] == -np.inf and prow[s + 1] == prow[s], s
            continue
        e_lq = abs(logq[s] - want["logq"]) / max(1.0, abs(want["logq"]))
        assert e_lq <= 1e-11, (s, logq[s], want["logq"])
        cap = PR.cap(want["logq"], L)
        for i in range(L):
            a, b = mrow[b0 + i], mrow[b0 + i + 1]
            assert (np.diff(midx[a:b]) > 0).all(), (s, i)   # ascending state ids
            got = np.zeros(n_states)
            got[midx[a:b]] = mval[a:b]
            e_m = np.abs(got - want["mass"][i]).max()
            assert e_m <= cap, (s, i, e_m, cap)
            listed = np.zeros(n_states, dtype=bool)
            listed[midx[a:b]] = True
            assert listed[want["mass"][i] > 1e-9].all(), (s, i)    # every state of some mass is listed
            assert (want["mass"][i][listed] > 0.0).all(), (s, i)   # and nothing of mass 0
            worst[0] = max(worst[0], e_m)
        e_b = np.abs(boundary[b0:b0 + L] - want["boundary"]).max() if L else 0.0
        assert e_b <= cap, (s, e_b, cap)
        worst[1], worst[2] = max(worst[1], e_b), max(worst[2], e_lq)
        if not decode:
            continue
        ids = pidx[prow[s]:prow[s + 1]]
        hits = [l for l in _match(entry, ids) if np.isfinite(want["lw"][l])]
        assert hits, (s, ids)   # one of the string's enumerated paths of finite weight
        l = hits[0]
        assert abs(plw[s] - want["lw"][l]) <= _tol(want["lw"][l]), (s, plw[s], want["lw"][l])
        e_s = min(abs(score[s] - want["score"][h]) for h in hits)
        assert e_s <= L * cap, (s, score[s], want["score"][l], L * cap)
        assert score[s] >= want["best"] - L * cap, (s, score[s], want["best"])
        assert 0.0 < score[s] <= L or L == 0, (s, score[s])
        if L:
            worst[3] = max(worst[3], e_s / (L * cap))
        if kbest is not None:   # where the path is among the k best, it carries their weight's bytes
            srow, klogw, kprow, kpidx = kbest
            for t in range(srow[s], srow[s + 1]):
                if kpidx[kprow[t]:kprow[t + 1]].tobytes() == ids.tobytes():
                    assert klogw[t:t + 1].tobytes() == plw[s:s + 1].tobytes(), (s, t)
    return worst


@pytest.mark.parametrize("name", CASES)
def test_masses_boundaries_and_decode_match_the_enumeration(name, monkeypatch):
    """three weight draws; wide200 has more than 64 destinations per byte
    (several lane rounds), long64 strings of 64 positions"""
    ref = _source(name)
    dev = _device(ref, monkeypatch)
    en = _enum(name)
    assert [e["n"] for e in en["strings"]] == [int(v) for v in ref["o"].path_counts()]
    if name == "wide200":
        assert dev.stats()["n_nodes"] > 64
    rng = np.random.default_rng(5)
    worst = [0.0, 0.0, 0.0, 0.0]
    for draw in range(3):
        x, w = _weights(ref, dev, rng)
        plain = dev.byte_marginals(w)
        assert plain[4].tobytes() == dev.posterior_counts(w)[3].tobytes()   # log q: posterior_counts' bytes
        full = dev.byte_marginals(w, decode=True)
        for u, v in zip(plain, full[:5]):
            assert u.tobytes() == v.tobytes()
        worst = [max(a, b) for a, b in zip(worst, _check(ref, en, w, full, kbest=dev.kbest_paths(w, 16)))]
    print("byte_marginals errors", name, "mass %.3e boundary %.3e logq %.3e score/(L cap) %.3e" % tuple(worst))
    assert dev.stats()["byte_marginal_ms"] > 0.0


def _ids(fsa):
    return {n: u for u, n in enumerate(fsa.state_names())}


def test_mea_differs_from_viterbi():
    """fixture (a): the case with power -- a decoder that maximises the path
    weight passes everything else and fails here"""
    dev, fsa, w = fixture_device(FIXTURE_A, named=FIXTURE_A_WEIGHTS)
    st = _ids(fsa)
    names = fsa.param_names()
    mrow, midx, mval, boundary, logq, score, plw, prow, pidx = dev.byte_marginals(w, decode=True)
    # (0.4, 0.6, ... are exp and log of doubles next to them: a few roundings of 1.1e-16 each, 1e-14 in all)
    eps = 1e-14
    assert abs(logq[0]) <= eps
    assert list(midx[mrow[0]:mrow[1]]) == sorted([st["A1"], st["B1"]])
    byte1 = dict(zip(midx[mrow[0]:mrow[1]], mval[mrow[0]:mrow[1]]))
    assert abs(byte1[st["A1"]] - 0.4) <= eps and abs(byte1[st["B1"]] - 0.6) <= eps
    byte2 = dict(zip(midx[mrow[1]:mrow[2]], mval[mrow[1]:mrow[2]]))
    assert set(byte2) == {st["A2"], st["C2"], st["D2"]}
    assert abs(byte2[st["A2"]] - 0.4) <= eps and abs(byte2[st["C2"]] - 0.35) <= eps and abs(byte2[st["D2"]] - 0.25) <= eps
    assert np.abs(boundary - 1.0).max() <= eps
    # Viterbi takes the A path, the MEA decode B1 - C2 with score 0.95 (A: 0.80, B1 - D2: 0.85)
    best, bprow, bpidx = dev.best_paths(w)
    assert [names[j] for j in bpidx[bprow[0]:bprow[1]]] == [("^", "T", "A1")]
    assert abs(best[0] - np.log(0.4)) <= eps
    assert [names[j] for j in pidx[prow[0]:prow[1]]] == [("^", "T", "B1"), ("B1", "T", "C2")]
    assert abs(score[0] - 0.95) <= 2 * eps and abs(plw[0] - np.log(0.35)) <= eps


def test_a_multi_byte_emission_is_exact():
    """fixture (b): both bytes of xy lie inside the one emission of X"""
    dev, fsa, w = fixture_device(FIXTURE_B)
    st = _ids(fsa)
    mrow, midx, mval, boundary, logq, score, plw, prow, pidx = dev.byte_marginals(w, decode=True)
    assert list(mrow) == [0, 1, 2] and list(midx) == [st["X"], st["X"]]
    assert mval.tobytes() == np.ones(2).tobytes()
    assert boundary.tobytes() == np.array([0.0, 1.0]).tobytes()
    assert score[0] == 2.0 and logq[0] == 0.0 and plw[0] == 0.0


def test_chain_nodes_carry_mass(monkeypatch):
    """test3 on aa: X emits a twice or aa once, so the boundary after byte 1 lies strictly between 0 and 1"""
    ref = _source("test3")
    dev = _device(ref, monkeypatch)
    _, w = _weights(ref, dev, np.random.default_rng(3))
    sym, off = np.asarray(ref["sym"], dtype=np.uint8).tobytes(), ref["off"]
    s = [sym[off[i]:off[i + 1]] for i in range(len(off) - 1)].index(b"aa")
    mrow, midx, mval, boundary, logq = dev.byte_marginals(w)
    assert 0.0 < boundary[off[s]] < 1.0 and boundary[off[s] + 1] == 1.0
    want = MR.derive(_enum("test3")["strings"][s], w, _enum("test3")["n_states"])
    assert abs(boundary[off[s]] - want["boundary"][0]) <= PR.cap(want["logq"], 2)


def test_single_path_strings_are_exact(monkeypatch):
    """compiled64: a string with exactly one path has one entry of exactly 1.0
    per byte, boundaries of exactly 1.0 (its emissions are single bytes), score
    exactly L and best_paths' path, byte for byte"""
    ref = _family("compiled64")
    dev = _device(ref, monkeypatch)
    _, w = _weights(ref, dev, np.random.default_rng(41))
    mrow, midx, mval, boundary, logq, score, plw, prow, pidx = dev.byte_marginals(w, decode=True)
    best, bprow, bpidx = dev.best_paths(w)
    en = _enum("compiled64")
    off = ref["off"]
    single = [s for s, e in enumerate(en["strings"]) if e["n"] == 1]
    assert len(single) >= 100
    for s in single:
        L = int(off[s + 1] - off[s])
        assert (np.diff(mrow[off[s]:off[s + 1] + 1]) == 1).all(), s
        assert (mval[mrow[off[s]]:mrow[off[s + 1]]] == 1.0).all(), s
        assert list(midx[mrow[off[s]]:mrow[off[s + 1]]]) == list(en["strings"][s]["states"][0]), s
        assert (boundary[off[s]:off[s + 1]] == 1.0).all(), s
        assert score[s] == float(L), (s, score[s])
        assert pidx[prow[s]:prow[s + 1]].tobytes() == bpidx[bprow[s]:bprow[s + 1]].tobytes(), s
        assert plw[s:s + 1].tobytes() == best[s:s + 1].tobytes(), s


@pytest.mark.parametrize("name", ["amb12", "long64", "test3"])
def test_a_dominant_path_is_the_mea_path(name, monkeypatch):
    """weights times 200 (as the sampler's test builds them): where the best
    path's posterior exp(logw - logq) exceeds 0.5, each of its bytes' states
    holds more than half the mass, so the MEA path's state sequence is the
    Viterbi path's (two paths with the same states tie in score: only the state
    sequences are compared)"""
    ref = _source(name)
    dev = _device(ref, monkeypatch)
    x, w = _weights(ref, dev, np.random.default_rng(41))
    w = 200.0 * w
    res = dev.byte_marginals(w, decode=True)
    logq, prow, pidx = res[4], res[7], res[8]
    best, bprow, bpidx = dev.best_paths(w)
    en = _enum(name)
    n = 0
    for s in range(len(best)):
        if not np.isfinite(best[s]) or not np.exp(best[s] - logq[s]) > 0.5:
            continue
        entry = en["strings"][s]
        vit = {entry["states"][l].tobytes() for l in _match(entry, bpidx[bprow[s]:bprow[s + 1]])}
        mea = {entry["states"][l].tobytes() for l in _match(entry, pidx[prow[s]:prow[s + 1]])}
        assert vit and mea and vit & mea, s
        n += 1
    assert n > 0


def test_deep_weights_keep_their_rows(monkeypatch):
    """long64 at x ~ N(-12, 0.5): q_s of the long strings lies below the double
    range (log q < -745); their rows stay within the cap and none is empty"""
    ref = _family("long64")
    dev = _device(ref, monkeypatch)
    x, w = _weights(ref, dev, np.random.default_rng(37), mean=-12.0)
    result = dev.byte_marginals(w, decode=True)
    print("byte_marginals errors long64_deep mass %.3e boundary %.3e logq %.3e score/(L cap) %.3e"
          % tuple(_check(ref, _enum("long64"), w, result)))
    mrow, logq, off = result[0], result[4], ref["off"]
    deep = np.flatnonzero(logq < -745.0)
    assert len(deep) > 0
    for s in deep:
        assert (np.diff(mrow[off[s]:off[s + 1] + 1]) > 0).all(), s


def test_minus_infinity_weights(monkeypatch):
    """the most-used quarter of amb12_seed7's used parameters at -inf (the
    posterior test's recipe): strings without a finite path own nothing, the rest
    agree with the enumeration without the -inf paths, no returned path touches a
    -inf parameter, and nothing is NaN but the boundaries and scores of the
    strings of mass 0"""
    ref = _family("amb12_seed7")
    dev = _device(ref, monkeypatch)
    P, trim = ref["P"], ref["trim"]
    x, w = _weights(ref, dev, np.random.default_rng(13))
    use = P.sum(axis=0)
    used = np.flatnonzero(use > 0)
    gone = used[np.argsort(-use[used], kind="stable")][:len(used) // 4]
    w = w.copy()
    w[np.isin(trim[dev.perm], gone)] = -np.inf
    en = _enum("amb12_seed7")
    finite = np.array([np.isfinite(MR.weights(e, w)).sum() if e["n"] else 0 for e in en["strings"]])
    paths = np.array([e["n"] for e in en["strings"]])
    assert (finite >= 1).any() and ((finite == 0) & (paths > 0)).any()
    result = dev.byte_marginals(w, decode=True)
    mrow, midx, mval, boundary, logq, score, plw, prow, pidx = result
    print("byte_marginals errors amb12_seed7_minus_inf mass %.3e boundary %.3e logq %.3e score/(L cap) %.3e"
          % tuple(_check(ref, en, w, result)))
    assert np.isfinite(w[pidx]).all()
    off = ref["off"]
    for s in range(len(finite)):
        sl = slice(off[s], off[s + 1])
        if finite[s] == 0:
            assert np.isnan(boundary[sl]).all() and np.isnan(score[s]) and plw[s] == -np.inf
        else:
            assert np.isfinite(boundary[sl]).all() and np.isfinite(score[s]) and np.isfinite(plw[s]) and np.isfinite(logq[s])
    assert np.isfinite(mval).all() and not np.isnan(logq).any() and not np.isnan(plw).any()


def test_more_strings_than_waves_and_the_same_bytes_again(monkeypatch):
    """9,000 strings on at most 4,096 waves, against the enumeration; a second
    call hands the tickets to other waves and returns the same bytes, and so
    does a call on 64 waves"""
    ref = _many()
    dev = _device(ref, monkeypatch)
    n_all = len(ref["off"]) - 1
    assert n_all == 9000 and n_all > 16 * 256
    x, w = _weights(ref, dev, np.random.default_rng(53))
    first = dev.byte_marginals(w, decode=True)
    print("byte_marginals errors many9000 mass %.3e boundary %.3e logq %.3e score/(L cap) %.3e"
          % tuple(_check(ref, _enum("many9000"), w, first)))
    second = dev.byte_marginals(w, decode=True)
    monkeypatch.setenv("WFSA_MARGINAL_WAVES", "64")
    third = dev.byte_marginals(w, decode=True)
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
        results.append(dev.byte_marginals(w, decode=True))
    _check(ref, _enum(name), w, results[1])
    for u, v in zip(*results):
        assert u.tobytes() == v.tobytes()


def test_byte_marginals_leave_the_quasinewton_loop_alone():
    """Run(3), Run(3) gives info rows bit-equal to Run(3), ByteMarginals(True), Run(3) (rmin column on)"""
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
            mrow, midx, mval, boundary, logq, score, plw, prow, pidx = lrn.ByteMarginals(True)
            assert np.isfinite(logq).all() and (np.diff(mrow) > 0).all() and (mval > 0.0).all()
            assert ((boundary >= 0.0) & (boundary <= 1.0)).all() and (score > 0.0).all() and (np.diff(prow) > 0).all()
            sums = np.add.reduceat(mval, mrow[:-1])
            assert np.abs(sums - 1.0).max() <= 1e-9
        rows += lrn.Run(3, 1.0, -1.0)
        runs.append(np.array(rows))
    assert runs[0].shape == (6, 7)
    assert runs[0].tobytes() == runs[1].tobytes()
    assert W.HessianLearner.ByteMarginals is W.QuasiNewtonLearner.ByteMarginals


def test_byte_marginals_leave_rmin_and_the_other_results_alone():
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
    dev.byte_marginals(w2, decode=True)
    assert dev.rmin() == plain
    # the four other results outlive a byte_marginals call ...
    _, bprow, bpidx = dev.best_paths(w1)
    kb = dev.kbest_paths(w1, 4)
    sp = dev.sample_paths(w1, 8, seed=1)
    pc = dev.posterior_counts(w1)
    bm = dev.byte_marginals(w2, decode=True)
    for u, v in zip((bprow, bpidx), _get(lib.wfsa_dev_best_paths_get, dev, (bprow, bpidx))):
        assert u.tobytes() == v.tobytes()
    for u, v in zip(kb, _get(lib.wfsa_dev_kbest_paths_get, dev, kb)):
        assert u.tobytes() == v.tobytes()
    for u, v in zip(sp[:4], _get(lib.wfsa_dev_sample_paths_get, dev, sp[:4])):
        assert u.tobytes() == v.tobytes()
    for u, v in zip(pc[:3], _get(lib.wfsa_dev_posterior_counts_get, dev, pc[:3])):
        assert u.tobytes() == v.tobytes()
    # ... and the other way round
    dev.best_paths(w1)
    dev.kbest_paths(w1, 4)
    dev.sample_paths(w1, 8, seed=1)
    dev.posterior_counts(w1)
    for u, v in zip(bm[:3], _get(lib.wfsa_dev_byte_marginals_get, dev, bm[:3])):
        assert u.tobytes() == v.tobytes()
    for u, v in zip(bm[7:], _get(lib.wfsa_dev_byte_marginals_path_get, dev, bm[7:])):
        assert u.tobytes() == v.tobytes()


def test_byte_marginals_errors(monkeypatch):
    import wfsa_amd as W
    from wfsa_amd import _lib
    lib = W.load()
    ref = _golden("talk", "talk")
    fsa = W.Fsa.read_text(ref["text"])
    # before a model and a corpus are loaded
    dev = W.Device(0)
    with pytest.raises(W.WfsaError) as e:
        dev.byte_marginals(np.zeros(0))
    assert e.value.code == _lib.WFSA_ERR_ARG
    dev.load_model(fsa)
    with pytest.raises(W.WfsaError) as e:
        dev.byte_marginals(np.zeros(dev.n_params))
    assert e.value.code == _lib.WFSA_ERR_ARG
    # _get without a result since the last load
    dev.load_corpus(ref["sym"], ref["off"], ref["wt"] / ref["wt"].sum())
    mrow = np.zeros(int(ref["off"][-1]) + 1, dtype=np.int64)
    prow = np.zeros(dev.n_strings + 1, dtype=np.int64)
    assert lib.wfsa_dev_byte_marginals_get(dev._h, mrow.ctypes.data_as(C.c_void_p), None, None) == _lib.WFSA_ERR_ARG
    assert lib.wfsa_dev_byte_marginals_path_get(dev._h, prow.ctypes.data_as(C.c_void_p), None) == _lib.WFSA_ERR_ARG
    # while an evaluation is in flight
    w = np.full(dev.n_params, -1.0)
    dev.objective_grad_begin(w)
    with pytest.raises(W.WfsaError) as e:
        dev.byte_marginals(w)
    assert e.value.code == _lib.WFSA_ERR_ARG and "in flight" in str(e.value)
    dev.objective_grad_end()
    # the paths belong to a call with the decode
    mrow2, midx, mval, boundary, logq = dev.byte_marginals(w)
    assert np.isfinite(logq).sum() == 3 and (logq == -np.inf).sum() == 2
    assert lib.wfsa_dev_byte_marginals_get(dev._h, mrow.ctypes.data_as(C.c_void_p), None, None) == 0
    assert mrow.tobytes() == mrow2.tobytes()
    assert lib.wfsa_dev_byte_marginals_path_get(dev._h, prow.ctypes.data_as(C.c_void_p), None) == _lib.WFSA_ERR_ARG
    assert "decode = 0" in lib.wfsa_dev_last_error().decode()
    res = dev.byte_marginals(w, decode=True)
    assert lib.wfsa_dev_byte_marginals_path_get(dev._h, prow.ctypes.data_as(C.c_void_p), None) == 0
    assert prow.tobytes() == res[7].tobytes() and (np.diff(prow) > 0).sum() == 3
    # a load drops the result
    dev.load_corpus(ref["sym"], ref["off"], ref["wt"] / ref["wt"].sum())
    assert lib.wfsa_dev_byte_marginals_get(dev._h, mrow.ctypes.data_as(C.c_void_p), None, None) == _lib.WFSA_ERR_ARG
    # matrix-file mode: no automaton
    dev.load_paths(2, [0, 1, 2], [0, 1], [1.0, 1.0], [0, 2], [0, 1], [1.0])
    with pytest.raises(W.WfsaError) as e:
        dev.byte_marginals(np.zeros(2))
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
        dd.byte_marginals(np.full(dd.n_params, -1.0))
    assert e.value.code == _lib.WFSA_ERR_CAPACITY and "WFSA_DENSE=0" in str(e.value)
