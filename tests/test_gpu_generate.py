"""GPU tests of unconditional generation (wfsa_dev_generate, generate.hip): n
strings drawn from the automaton itself, with their paths and weights, against
the numpy walker of the contract (generate_reference.py).

A sample without a near-tie flag (no choice within 1e-9 T of a running sum,
where one ulp in exp could pick another candidate) must equal the reference in
bytes, path and status, with logw to 1e-12 max(1, |logw|) and logp to
1e-12 (steps + 1); the lane, wave and block edges, the choice rule on
hand-written automata, the cap, dead mass, the distribution at group-normalised
weights against log q from objective_grad, the agreement with the decoders,
the dense path, the isolation from the learning path and the errors of the
contract in include/wfsa_dev.h follow.  Needs a gfx950 device."""
import ctypes as C
import os

import numpy as np
import pytest

import generate_reference as G
import sample_reference as R
from conftest import DATA
from decode_cases import _big, _family, _tol

pytestmark = pytest.mark.gpu


def _text(name):
    if name == "test.loop":
        return open(os.path.join(DATA, "test.loop.wfsa"), "rb").read().decode("latin-1")
    return _family(name)["text"]


def _dev(text):
    import wfsa_amd as W
    fsa = W.Fsa.read_text(text)
    dev = W.Device(0)
    dev.load_model(fsa)
    return dev, fsa


def _ids(out, i):
    return out["pidx"][out["prow"][i]:out["prow"][i + 1]]


def _bytes(out, i):
    return out["sym"][out["off"][i]:out["off"][i + 1]].tobytes()


def _layout(out, n):
    for key, data in (("off", "sym"), ("prow", "pidx")):
        row = out[key]
        assert row.shape == (n + 1,) and row[0] == 0 and row[-1] == len(out[data]) and (np.diff(row) >= 0).all()
    assert out["logw"].shape == out["logp"].shape == out["status"].shape == (n,)
    assert set(np.unique(out["status"])) <= {0, 1, 2}


def _same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("sym", "off", "logw", "logp", "status", "prow", "pidx"))


def _parity(got, ref, n):
    """every unflagged sample equals the reference; returns the flagged count"""
    _layout(got, n)
    ok = np.flatnonzero(~ref["near"])
    for i in ok:
        assert got["status"][i] == ref["status"][i], i
        assert _bytes(got, i) == _bytes(ref, i), i
        assert _ids(got, i).tobytes() == _ids(ref, i).tobytes(), i
    assert (np.abs(got["logw"][ok] - ref["logw"][ok]) <= 1e-12 * np.maximum(1.0, np.abs(ref["logw"][ok]))).all()
    assert (np.abs(got["logp"][ok] - ref["logp"][ok]) <= 1e-12 * (ref["steps"][ok] + 1)).all()
    if len(ok) == n:
        assert got["off"].tobytes() == ref["off"].tobytes() and got["prow"].tobytes() == ref["prow"].tobytes()
    return n - len(ok)


@pytest.mark.parametrize("name", ["amb12", "test.loop"])
def test_parity_with_the_reference(name):
    dev, fsa = _dev(_text(name))
    rng = np.random.default_rng(11)
    n = 4096
    for draw in range(3):
        w = rng.normal(-1.0, 0.5, size=dev.n_params)
        got = dev.generate(w, n, max_len=8, seed=draw)
        ref = G.generate(fsa, w, n, 8, draw)
        flagged = _parity(got, ref, n)
        print(name, "draw", draw, "flagged", flagged, "status", np.bincount(got["status"], minlength=3))
        assert flagged <= n // 1000
        assert (got["status"] == 0).any()
    assert dev.stats()["generate_ms"] > 0.0


def test_lane_wave_and_block_edges():
    dev, fsa = _dev(_text("amb12"))
    w = np.random.default_rng(13).normal(-1.0, 0.5, size=dev.n_params)
    whole = dev.generate(w, 257, max_len=8, seed=9)
    ref = G.generate(fsa, w, 257, 8, 9)
    assert not ref["near"].any()
    assert _parity(whole, ref, 257) == 0
    for n in (1, 63, 64, 65, 257):
        got = dev.generate(w, n, max_len=8, seed=9)
        _layout(got, n)
        # the first n samples of the 257 result, byte for byte
        assert got["off"].tobytes() == whole["off"][:n + 1].tobytes() and got["prow"].tobytes() == whole["prow"][:n + 1].tobytes()
        assert got["sym"].tobytes() == whole["sym"][:whole["off"][n]].tobytes()
        assert got["pidx"].tobytes() == whole["pidx"][:whole["prow"][n]].tobytes()
        for k in ("logw", "logp", "status"):
            assert got[k].tobytes() == whole[k][:n].tobytes()
    assert _same(dev.generate(w, 257, max_len=8, seed=9), whole)
    assert not _same(dev.generate(w, 257, max_len=8, seed=10), whole)


@pytest.mark.parametrize("k", [1, 2, 65, 130])
def test_choice_groups(k):
    """a transition group of k: param -1 (k = 1), 2, and 65 / 130, where the
    bisection takes 7 and 8 probes; the first and the last member are taken as
    often as the reference takes them"""
    dev, fsa = _dev(G.fan(k))
    group = G.params_of(fsa, "^", "T")
    assert len(group) == k and (dev.n_params == 0) == (k == 1) and ((group == -1).all() if k == 1 else (group >= 0).all())
    w = np.random.default_rng(k).normal(-1.0, 0.3, size=dev.n_params)
    n = 4096
    got = dev.generate(w, n, max_len=4, seed=k)
    ref = G.generate(fsa, w, n, 4, k)
    assert not ref["near"].any()
    assert _parity(got, ref, n) == 0
    assert (got["status"] == 0).all() and (np.diff(got["off"]) == 2).all()
    if k == 1:
        assert len(got["pidx"]) == 0 and (got["logw"] == 0.0).all() and (got["logp"] == 0.0).all()
        return
    assert (np.diff(got["prow"]) == 1).all()
    taken, want = np.bincount(got["pidx"], minlength=dev.n_params), np.bincount(ref["pidx"], minlength=dev.n_params)
    for member in (group[0], group[-1]):
        assert taken[member] == want[member] > 0, (member, taken[member], want[member])
    # logp = w_k - log T, T the group's left-to-right sum
    T = G.running_sums(np.array([0, k]), group, w)[-1]
    assert (np.abs(got["logp"] - (w[got["pidx"]] - np.log(T))) <= 2e-12).all()


def test_emissions_and_the_cap():
    dev, fsa = _dev(G.EMISSIONS)
    w = fsa.weights()
    n = 4096
    three, empty = G.emission_param(fsa, "B", b"def"), G.emission_param(fsa, "A", b"")
    for max_len in (0, 1, 2, 7):
        got = dev.generate(w, n, max_len=max_len, seed=max_len)
        ref = G.generate(fsa, w, n, max_len, max_len)
        assert not ref["near"].any()
        assert _parity(got, ref, n) == 0
        lens = np.diff(got["off"])
        assert (lens <= max_len).all() and (got["status"] != 2).all()
        done, cut = got["status"] == 0, got["status"] == 1
        assert done.any() and cut.any()
        if max_len == 0:   # only the empty string completes: ^ -> A (empty)* -> $
            assert (lens == 0).all() and len(got["sym"]) == 0
        if max_len == 7:   # an epsilon step, and emissions of 1, 2 and 3 bytes
            strs = [_bytes(got, i) for i in np.flatnonzero(done)]
            assert b"" in strs and any(b"bc" in s for s in strs) and any(b"def" in s for s in strs) and any(b"a" in s for s in strs)
            assert (got["pidx"] == empty).any()
        if max_len == 2:   # "def" never fits: cut at its second byte, absent from bytes and path
            assert b"d" not in got["sym"].tobytes() and not (got["pidx"] == three).any()
            # a walk at "a" that enters B is cut at the second byte of "bc" or "def": it keeps "a" and the transition
            ab = G.transition_param(fsa, "A", "B")
            assert any(_bytes(got, i) == b"a" and _ids(got, i)[-1] == ab for i in np.flatnonzero(cut))
        # a truncated sample's weights are those of the recorded choices
        for i in np.flatnonzero(cut)[:50]:
            assert abs(w[_ids(got, i)].sum() - got["logw"][i]) <= _tol(got["logw"][i])


def test_dead_mass():
    dev, fsa = _dev(G.TINY)
    w = fsa.weights()
    n = 4096
    # all of B's emissions at -inf: exactly the walks that reach B die
    ww = w.copy()
    ww[G.params_of(fsa, "B", "E")] = -np.inf
    got = dev.generate(ww, n, max_len=8, seed=1)
    ref = G.generate(fsa, ww, n, 8, 1)
    assert not ref["near"].any() and _parity(got, ref, n) == 0
    into_b = {G.transition_param(fsa, "^", "B"), G.transition_param(fsa, "A", "B")}
    dead = got["status"] == 2
    assert dead.any() and (~dead).any() and (got["status"] != 1).all()
    for i in range(n):
        ids = _ids(got, i)
        assert dead[i] == (len(ids) > 0 and int(ids[-1]) in into_b), i
    assert np.isfinite(got["logw"]).all() and np.isfinite(got["logp"]).all()
    # one candidate at -inf: never chosen
    for kind, state in (("T", "A"), ("E", "B"), ("T", "^")):
        ww = w.copy()
        off = G.params_of(fsa, state, kind)[0]
        ww[off] = -np.inf
        got = dev.generate(ww, n, max_len=8, seed=2)
        assert not (got["pidx"] == off).any() and (got["status"] == 0).all()
        assert _parity(got, G.generate(fsa, ww, n, 8, 2), n) == 0


@pytest.mark.parametrize("seed", G.DIST_SEEDS)
def test_samples_follow_the_model(seed):
    """amb12 at group-normalised weights, 65,536 samples: the distinct strings'
    counts against n exp(log q_s), log q_s from objective_grad on the distinct
    strings; cells with expectation below 5 and the truncated and dead samples
    in one rest cell; X^2 <= dof + 6 sqrt(2 dof) (test_generate_reference.py
    shows the reference passes it for these seeds)"""
    import wfsa_amd as W
    text, w = G.dist_model()
    fsa = W.Fsa.read_text(text)
    dev = W.Device(0)
    dev.load_model(fsa)
    n = G.DIST_N
    got = dev.generate(w, n, max_len=G.DIST_MAX_LEN, seed=seed)
    _layout(got, n)
    assert (np.abs(got["logw"] - got["logp"]) <= 1e-12 * (2 * G.DIST_MAX_LEN + 4)).all()   # every group sums to 1
    sym, off, counts = got.distinct()
    assert counts.sum() == (got["status"] == 0).sum()
    dev.load_corpus(sym, off, counts / counts.sum())
    rec, _, _ = dev.recognize()
    assert rec.all()
    _, _, logq = dev.objective_grad(w, want_logq=True)
    assert np.isfinite(logq).all()   # no sample on a string of probability 0
    x2, dof = G.chi_square(counts, n * np.exp(logq), int((got["status"] != 0).sum()), n)
    print("seed", seed, "X^2", x2, "dof", dof, "bound", R.bound(dof), "distinct", len(counts))
    assert dof >= 100
    assert x2 <= R.bound(dof), (x2, dof)


def test_agreement_with_the_decoders():
    """compiled64: the distinct complete strings as a corpus are all
    recognized; a sampled path of a string with at most 16 paths is a
    kbest_paths(16) entry with the same ids and its weight to 1e-12; and
    logw <= log q (to the rounding of two sums of at most 64 terms formed in
    different orders: 64 * 2^-53 max(1, |log q|))"""
    dev, fsa = _dev(_family("compiled64")["text"])
    w = np.random.default_rng(17).normal(-1.0, 0.5, size=dev.n_params)
    n = 2048
    got = dev.generate(w, n, max_len=12, seed=3)
    sym, off, counts = got.distinct()
    strs = [sym[off[s]:off[s + 1]].tobytes() for s in range(len(counts))]
    assert len(strs) > 50
    dev.load_corpus(sym, off, counts / counts.sum())
    rec, pc, _ = dev.recognize()
    assert rec.all()
    _, _, logq = dev.objective_grad(w, want_logq=True)
    ks, kl, kp, ki = dev.kbest_paths(w, 16)
    row = {s: r for r, s in enumerate(strs)}
    checked = 0
    for i in np.flatnonzero(got["status"] == 0):
        r = row[_bytes(got, i)]
        assert got["logw"][i] <= logq[r] + 64 * 2.0 ** -53 * max(1.0, abs(logq[r])), (i, got["logw"][i], logq[r])
        if pc[r] > 16:
            continue
        entries = {ki[kp[t]:kp[t + 1]].tobytes(): kl[t] for t in range(ks[r], ks[r + 1])}
        ids = _ids(got, i).tobytes()
        assert ids in entries, (i, r)
        assert abs(entries[ids] - got["logw"][i]) <= _tol(got["logw"][i]), (i, entries[ids], got["logw"][i])
        checked += 1
    assert checked > n // 4 and (pc[pc <= 16] > 1).any()
    # generation needs no corpus, and the corpus loaded since does not change it
    assert _same(dev.generate(w, n, max_len=12, seed=3), got)


def test_dense_path_generates(monkeypatch):
    import wfsa_amd as W
    syn = W.Synthetic(n_states=16, degree=1, vocab=6, emissions=2, dense=True, n_strings=50, max_len=9, seed=3)
    out = []
    for dense in ("1", "0"):
        monkeypatch.setenv("WFSA_DENSE", dense)
        dev = W.Device(0)
        dev.load_model(W.Fsa.read_text(syn.wfsa_text))
        assert dev.stats()["dense"] == int(dense)
        w = np.random.default_rng(19).normal(-1.0, 0.5, size=dev.n_params)
        out.append(dev.generate(w, 1000, max_len=9, seed=4))
        if dense == "1":   # with the corpus on the dense path as well
            sym, off, wt = syn.corpus()
            dev.load_corpus(sym, off, wt / wt.sum())
            assert dev.stats()["dense"] == 1
            assert _same(dev.generate(w, 1000, max_len=9, seed=4), out[0])
    assert _same(out[0], out[1]) and (out[0]["status"] == 0).any()
    fsa = W.Fsa.read_text(syn.wfsa_text)
    ref = G.generate(fsa, w, 1000, 9, 4)
    assert _parity(out[0], ref, 1000) <= 1


def test_generate_leaves_the_quasinewton_loop_alone():
    """Run(3), Run(3) gives info rows bit-equal to Run(3), Generate(500), Run(3) (rmin column on)"""
    import wfsa_amd as W
    fsa, sym, off, wt = _big()
    runs = []
    for gen in (False, True):
        lrn = W.QuasiNewtonLearner(0)
        lrn.set_info_rmin(True)
        lrn.BuildFromPacked(fsa, sym, off, wt)
        lrn.Finalize()
        lrn.Init(7)
        rows = lrn.Run(3, 1.0, -1.0)
        if gen:
            out = lrn.Generate(500, max_len=64, seed=6)
            _layout(out, 500)
            assert (out["status"] == 0).any() and np.isfinite(out["logw"]).all()
            assert _same(lrn.Generate(500, max_len=64, seed=6), out)
        rows += lrn.Run(3, 1.0, -1.0)
        runs.append(np.array(rows))
    assert runs[0].shape == (6, 7)
    assert runs[0].tobytes() == runs[1].tobytes()
    assert W.HessianLearner.Generate is W.QuasiNewtonLearner.Generate


def _get(fn, dev, like):
    out = [np.zeros_like(v) for v in like]
    assert fn(dev._h, *(v.ctypes.data_as(C.c_void_p) for v in out)) == 0
    return out


def test_generate_leaves_the_other_results_alone():
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
    dev.objective_grad(w1, want_logq=False)
    dev.generate(w2, 300, max_len=32, seed=1)
    assert dev.rmin() == plain
    _, bprow, bpidx = dev.best_paths(w1)
    sp = dev.sample_paths(w1, 4, seed=1)
    gen = dev.generate(w2, 300, max_len=32, seed=1)
    for u, v in zip((bprow, bpidx), _get(lib.wfsa_dev_best_paths_get, dev, (bprow, bpidx))):
        assert u.tobytes() == v.tobytes()
    for u, v in zip(sp[:4], _get(lib.wfsa_dev_sample_paths_get, dev, sp[:4])):
        assert u.tobytes() == v.tobytes()
    # ... and the other way round
    dev.best_paths(w2)
    dev.sample_paths(w2, 4, seed=2)
    keys = ("sym", "off", "logw", "logp", "status", "prow", "pidx")
    for k, v in zip(keys, _get(lib.wfsa_dev_generate_get, dev, [gen[k] for k in keys])):
        assert gen[k].tobytes() == v.tobytes(), k


def test_generate_errors(monkeypatch):
    import wfsa_amd as W
    from wfsa_amd import _lib
    lib = W.load()

    def refused(dev, w, n=4, max_len=8, word=None):
        with pytest.raises(W.WfsaError) as e:
            dev.generate(w, n, max_len=max_len)
        assert e.value.code == _lib.WFSA_ERR_ARG and (word is None or word in str(e.value)), str(e.value)

    # before a model is loaded
    dev = W.Device(0)
    refused(dev, np.zeros(0))
    off = np.zeros(5, dtype=np.int64)
    assert lib.wfsa_dev_generate_get(dev._h, None, off.ctypes.data_as(C.c_void_p), None, None, None, None, None) == _lib.WFSA_ERR_ARG
    text = _family("amb12")["text"]
    fsa = W.Fsa.read_text(text)
    dev.load_model(fsa)
    w = np.full(dev.n_params, -1.0)
    # _get without a result since the last load
    assert lib.wfsa_dev_generate_get(dev._h, None, off.ctypes.data_as(C.c_void_p), None, None, None, None, None) == _lib.WFSA_ERR_ARG
    # n < 1, max_len < 0, a draw index past 32 bits
    refused(dev, w, n=0, word="n = 0")
    refused(dev, w, n=-3)
    refused(dev, w, max_len=-1, word="max_len")
    n_states = fsa.counts()["states"]
    refused(dev, w, max_len=2 ** 31 // n_states, word="draw")
    # a NaN and a +inf weight
    for bad in (np.nan, np.inf):
        ww = w.copy()
        ww[dev.n_params // 2] = bad
        refused(dev, ww, word="NaN or +inf")
    assert lib.wfsa_dev_generate_get(dev._h, None, off.ctypes.data_as(C.c_void_p), None, None, None, None, None) == _lib.WFSA_ERR_ARG
    got = dev.generate(w, 4, max_len=8)
    assert lib.wfsa_dev_generate_get(dev._h, None, off.ctypes.data_as(C.c_void_p), None, None, None, None, None) == 0
    assert off.tobytes() == got["off"].tobytes()
    # while an evaluation is in flight
    ref = _family("amb12")
    dev.load_corpus(ref["sym"], ref["off"], ref["wt"] / ref["wt"].sum())
    assert lib.wfsa_dev_generate_get(dev._h, None, off.ctypes.data_as(C.c_void_p), None, None, None, None, None) == _lib.WFSA_ERR_ARG
    dev.objective_grad_begin(w)
    refused(dev, w, word="in flight")
    dev.objective_grad_end()
    # matrix-file mode: no automaton
    dev.load_paths(2, [0, 1, 2], [0, 1], [1.0, 1.0], [0, 2], [0, 1], [1.0])
    refused(dev, np.zeros(2), word="matrix")
    # every output pointer may be NULL
    dev.load_model(fsa)
    assert lib.wfsa_dev_generate(dev._h, w.ctypes.data_as(C.c_void_p), 10, 8, 0, None, None, None) == 0
    assert lib.wfsa_dev_generate_get(dev._h, None, None, None, None, None, None, None) == 0
