"""GPU tests of the byte marginals and the MEA decode on the dense path
(wfsa_dev_dense_byte_marginals, dense_marginals.hip): the masses against the
log-domain numpy restatement (dense_marginal_reference.py) within the
project's cap 3e-11 * max(1, |log q|) * (L + 1), against the trellis tier of
the same model under WFSA_DENSE=0, the decode bit for bit as a function of the
device's own stored masses (mea_replay), log q byte for byte against
objective_grad and dense_sample_paths, every engine, repeatability, strings
without a path, the results that must survive, the learner and the CLI, errors
and stats.  Per case one call's results are shared by the tests that read them.
The worst errors are printed as one JSON line when the module ends
(profiles/dense_byte_marginals/errors.json).  The two capacity errors (a history
that cannot be allocated, more than 4 GiB of rows) have no test: they need a
failed allocation or 4 GiB of rows.  Needs a gfx950 device."""
import json
import os
import subprocess

import numpy as np
import pytest

import dense_decode_reference as R
import dense_marginal_reference as M
import dense_sample_reference as D
from conftest import ROOT

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "w-fsa_amd", "wfsa_amd", "wfsa")
LOGQ_REL = 1e-12   # test_gpu_dense.py's bound on log q against its reference
CASES = ("dense16", "auto128", "tiles200", "slots64") + D.GADGET_CASES + ("without_a_path",)
ERRORS = {}
_RUNS = {}


@pytest.fixture(scope="module", autouse=True)
def _report_and_drop():
    yield
    print("dense_byte_marginals errors " + json.dumps({k: ERRORS[k] for k in sorted(ERRORS)}, sort_keys=True))
    _RUNS.clear()
    M.clear_caches()


def _note(name, **errs):
    worst = ERRORS.setdefault(name, {})
    for k, v in errs.items():
        worst[k] = max(worst.get(k, 0.0), float(v))
    print(f"dense_byte_marginals worst | {name} | " + " ".join(f"{k} {v:.3e}" for k, v in sorted(worst.items())))


def _device(fsa, sym, off, p, monkeypatch, dense=True):
    """dense: True forced, False the trellis tiers, None chosen by the library"""
    import wfsa_amd as W
    if dense is None:
        monkeypatch.delenv("WFSA_DENSE", raising=False)
    else:
        monkeypatch.setenv("WFSA_DENSE", "1" if dense else "0")
    dev = W.Device(0)
    dev.load_model(fsa)
    dev.load_corpus(sym, off, p)
    assert dev.stats()["dense"] == (0 if dense is False else 1)
    return dev


def _same_bytes(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert u.dtype == v.dtype and u.shape == v.shape
        assert u.tobytes() == v.tobytes()


def _run(name, monkeypatch):
    """dense_byte_marginals(rows, decode) of a case on the default engine, once:
    (result, stats)"""
    if name not in _RUNS:
        monkeypatch.delenv("WFSA_DENSE_ENGINE", raising=False)
        monkeypatch.delenv("WFSA_DENSE_BLAS", raising=False)
        fsa, w, sym, off, p = M.expected(name)[:5]
        dev = _device(fsa, sym, off, p, monkeypatch, dense=None if name == "auto128" else True)
        res = dev.dense_byte_marginals(w, rows=True, decode=True)
        for a in res:
            a.setflags(write=False)
        _RUNS[name] = (res, dev.stats())
    return _RUNS[name]


def _stored(fsa, res, off, s, n_cols=None, ids=None):
    """string s's rows as an array [L][columns]: column = interior index (ids
    given: the interior states' Fsa ids) or Fsa state id; 0.0 where unlisted"""
    mrow, midx, mval = res[:3]
    a, b = int(off[s]), int(off[s + 1])
    out = np.zeros((b - a, n_cols))
    e0, e1 = int(mrow[a]), int(mrow[b])
    byte = np.repeat(np.arange(b - a), np.diff(mrow[a:b + 1]))
    col = midx[e0:e1]
    if ids is not None:
        inv = np.full(int(ids.max()) + 1, -1)
        inv[ids] = np.arange(len(ids))
        col = inv[col]
        assert (col >= 0).all()
    out[byte, col] = mval[e0:e1]
    return out


def _check_masses(name, res):
    fsa, w, sym, off, p, tab, rlogq, rmass = M.expected(name)
    mrow, midx, mval, boundary, logq = res[:5]
    ids = M.state_ids(fsa)
    S = len(off) - 1
    assert len(mrow) == off[-1] + 1 and mrow[0] == 0 and mrow[-1] == len(midx) == len(mval)
    assert (np.diff(mrow) >= 0).all()
    assert ((mval > 0.0) & (mval <= 1.0)).all()
    assert np.isin(midx, ids).all()
    inner = np.ones(len(midx), dtype=bool)   # entries that are not the first of their byte: ascending ids
    inner[mrow[:-1][np.diff(mrow) > 0]] = False
    assert (np.diff(midx)[inner[1:]] > 0).all()
    none = np.isneginf(rlogq)
    assert np.array_equal(np.isneginf(logq), none)
    np.testing.assert_allclose(logq[~none], rlogq[~none], rtol=LOGQ_REL)
    e_mass = e_sum = e_rel = 0.0
    for s in range(S):
        L = int(off[s + 1] - off[s])
        if none[s]:
            assert mrow[off[s]] == mrow[off[s + 1]]
            assert np.isnan(boundary[off[s]:off[s + 1]]).all()
            continue
        assert (boundary[off[s]:off[s + 1]] == 1.0).all()
        if L == 0:
            continue
        c = M.cap(rlogq[s], L)
        got = _stored(fsa, res, off, s, tab.n, ids)
        err = np.abs(got - rmass[s]).max()       # listed: |mval - ref|; unlisted: the reference mass itself
        rows = np.abs(got.sum(axis=1) - 1.0).max()
        assert err <= c and rows <= c, (name, s, err, rows, c)
        assert (np.diff(mrow[off[s]:off[s + 1] + 1]) > 0).all()
        e_mass, e_sum, e_rel = max(e_mass, err), max(e_sum, rows), max(e_rel, err / c)
    _note(name, mass=e_mass, row_sum=e_sum, mass_over_cap=e_rel,
          logq_rel=np.abs(logq[~none] / rlogq[~none] - 1.0).max(initial=0.0))


def _check_decode(name, res):
    """pidx equal, score and path_logw equal as bytes, for every string"""
    fsa, w, sym, off, p, tab, rlogq, rmass = M.expected(name)
    mrow, midx, mval, boundary, logq, score, plw, prow, pidx = res
    ids = M.state_ids(fsa)
    assert len(prow) == len(off) and prow[0] == 0 and prow[-1] == len(pidx)
    for s in range(len(off) - 1):
        bytes_ = sym[off[s]:off[s + 1]]
        stored = _stored(fsa, res, off, s, tab.n, ids) if logq[s] > -np.inf else None
        states, want, sc, lw = M.mea_replay(tab, bytes_, stored)
        assert np.array_equal(pidx[prow[s]:prow[s + 1]], want), (name, s)
        assert score[s:s + 1].tobytes() == np.array([sc]).tobytes(), (name, s, score[s], sc)
        assert plw[s:s + 1].tobytes() == np.array([lw]).tobytes(), (name, s, plw[s], lw)
        if stored is None:
            assert np.isnan(score[s]) and plw[s] == -np.inf and prow[s] == prow[s + 1]
        elif len(bytes_):
            assert 0.0 < score[s] <= len(bytes_) * (1.0 + 1e-9)


@pytest.mark.parametrize("name", CASES)
def test_masses_equal_the_restatement(name, monkeypatch):
    """dense16 one tile; auto128 admitted by the library's own rule; tiles200
    np = 256, two column tiles, padded states, several strings per slot;
    slots64 several row tiles; the gadgets; strings without a path"""
    res, st = _run(name, monkeypatch)
    _check_masses(name, res)
    if name == "tiles200":
        assert st["dense_np"] == 256 and len(M.expected(name)[4]) > st["dense_rows"]
    if name == "slots64":
        assert st["dense_rows"] >= 256
    if name == "edge129":
        assert st["dense_np"] == 256


@pytest.mark.parametrize("name", CASES)
def test_the_decode_is_the_replay_of_the_stored_masses_bit_for_bit(name, monkeypatch):
    res, st = _run(name, monkeypatch)
    _check_decode(name, res)


def _full(fsa, res, off, s):
    return _stored(fsa, res, off, s, fsa.desc().n_states)


@pytest.mark.parametrize("name", ["dense16", "auto128"])
def test_against_the_trellis_tier(name, monkeypatch):
    """the same model under WFSA_DENSE=0: masses within twice the cap, the
    trellis boundary 1.0 (within the cap: below), scores within L x cap, each tier's path rescored
    with the other's masses reaches the other's score within that bound (paths
    are not compared: the tie orders differ)"""
    fsa, w, sym, off, p, tab, rlogq, rmass = M.expected(name)
    dn, _ = _run(name, monkeypatch)
    tr = _device(fsa, sym, off, p, monkeypatch, dense=False).byte_marginals(w, decode=True)
    ids = M.state_ids(fsa)
    # every interior state emits one byte, so an emission ends with every byte: the trellis boundary is 1 -- as the
    # trellis tier forms it, the sum of its 2^-62 fixed-point masses over the byte's state nodes, which lands an ulp
    # or so beside 1.0 on ambiguous strings (measured: see the module's JSON line), so it is held to the cap of a
    # mass, as test_gpu_byte_marginals.py holds it; the dense tier's own boundary is exactly 1.0
    assert (dn[3] == 1.0).all()
    e_bound = np.abs(tr[3] - 1.0)
    assert (e_bound <= np.repeat([M.cap(tr[4][s], off[s + 1] - off[s]) for s in range(len(off) - 1)], np.diff(off))).all()
    _note(name + " vs trellis", trellis_boundary_minus_one=e_bound.max(), trellis_boundaries_not_exactly_one=(tr[3] != 1.0).sum())
    np.testing.assert_allclose(dn[4], tr[4], rtol=LOGQ_REL)
    e_mass = e_score = 0.0
    for s in range(len(off) - 1):
        L = int(off[s + 1] - off[s])
        c = M.cap(tr[4][s], L)
        a, b = _full(fsa, dn, off, s), _full(fsa, tr, off, s)
        err = np.abs(a - b).max()
        assert err <= 2 * c, (s, err, c)
        assert abs(dn[5][s] - tr[5][s]) <= L * c
        bytes_ = sym[off[s]:off[s + 1]]
        d_states = M.path_states(tab, bytes_, dn[8][dn[7][s]:dn[7][s + 1]])
        t_states = M.path_states(tab, bytes_, tr[8][tr[7][s]:tr[7][s + 1]])
        assert d_states is not None and t_states is not None
        assert M.path_score(b[:, ids], d_states) >= tr[5][s] - L * c
        assert M.path_score(a[:, ids], t_states) >= dn[5][s] - L * c
        e_mass, e_score = max(e_mass, err / c), max(e_score, abs(dn[5][s] - tr[5][s]) / (L * c))
    _note(name + " vs trellis", mass_over_cap=e_mass, score_over_L_cap=e_score)


@pytest.mark.parametrize("name", ["holes12", "without_a_path"])
def test_the_empty_string_against_the_trellis_tier(name, monkeypatch):
    """holes12: an empty string with a ^ -> $ edge; without_a_path: one
    without.  Score, weight and path as the trellis byte_marginals returns
    them; no rows either way"""
    fsa, w, sym, off, p = M.expected(name)[:5]
    dn, _ = _run(name, monkeypatch)
    tr = _device(fsa, sym, off, p, monkeypatch, dense=False).byte_marginals(w, decode=True)
    empty = np.flatnonzero(np.diff(off) == 0)
    assert len(empty) > 0
    for s in empty:
        for k in (5, 6):   # score, path_logw
            assert dn[k][s:s + 1].tobytes() == tr[k][s:s + 1].tobytes(), (k, dn[k][s], tr[k][s])
        # log q: log(exp(w)) here, w there
        assert dn[4][s] == tr[4][s] or abs(dn[4][s] - tr[4][s]) <= LOGQ_REL * abs(tr[4][s])
        assert np.array_equal(dn[8][dn[7][s]:dn[7][s + 1]], tr[8][tr[7][s]:tr[7][s + 1]])
    if name == "holes12":
        assert np.isfinite(dn[4][empty]).all() and (dn[5][empty] == 0.0).all()
    else:
        assert np.isneginf(dn[4][empty]).all() and np.isnan(dn[5][empty]).all()


def test_the_mea_path_is_not_the_viterbi_path_on_the_device(monkeypatch):
    """dense16: at least one string's MEA path differs from dense_best_paths';
    for every string the MEA score is at least the Viterbi path's under the
    device's own masses"""
    fsa, w, sym, off, p, tab, rlogq, rmass = M.expected("dense16")
    res, _ = _run("dense16", monkeypatch)
    dev = _device(fsa, sym, off, p, monkeypatch)
    best_logw, brow, bidx = dev.dense_best_paths(w)
    ids = M.state_ids(fsa)
    differ = 0
    for s in range(len(off) - 1):
        bytes_ = sym[off[s]:off[s + 1]]
        vit = bidx[brow[s]:brow[s + 1]]
        stored = _stored(fsa, res, off, s, tab.n, ids)
        assert res[5][s] >= M.path_score(stored, M.path_states(tab, bytes_, vit))
        assert res[6][s] <= best_logw[s]
        differ += not np.array_equal(vit, res[8][res[7][s]:res[7][s + 1]])
    print("dense16: MEA path differs from dense_best_paths' on", differ, "of", len(off) - 1, "strings")
    assert differ >= 1


def test_logq_is_objective_grads_and_the_samplers_byte_for_byte(monkeypatch):
    """on a context running the default engine"""
    monkeypatch.delenv("WFSA_DENSE_ENGINE", raising=False)
    monkeypatch.delenv("WFSA_DENSE_BLAS", raising=False)
    for name in ("dense16", "tiles200"):
        fsa, w, sym, off, p = M.expected(name)[:5]
        dev = _device(fsa, sym, off, p, monkeypatch)
        dev.recognize()
        _, _, logq = dev.objective_grad(w, want_logq=True)
        got = dev.dense_byte_marginals(w, rows=False, decode=True)[4]
        assert got.tobytes() == np.asarray(logq, dtype=np.float64).tobytes()
        assert got.tobytes() == dev.dense_sample_paths(w, 1, 3)[4].tobytes()
        assert got.tobytes() == _run(name, monkeypatch)[0][4].tobytes()   # (before any evaluation has run on the context)


@pytest.mark.parametrize("engine", ["fused", "blas", "dma"])
def test_the_same_flow_on_every_engine(engine, monkeypatch):
    """whatever GEMM engine the context's evaluations run, the call runs the
    split-K flow: the bytes of a default-engine context (two column tiles)"""
    fsa, w, sym, off, p = M.expected("edge129")[:5]
    want, _ = _run("edge129", monkeypatch)
    monkeypatch.setenv("WFSA_DENSE_ENGINE", engine)
    dev = _device(fsa, sym, off, p, monkeypatch)
    assert dev.stats()["dense_blas"] != 2   # (not the split-K engine)
    dev.recognize()
    dev.objective_grad(w)   # (the engine's own buffers in use)
    _same_bytes(want, dev.dense_byte_marginals(w, rows=True, decode=True))


def test_repeat_and_the_decode_alone(monkeypatch):
    """two calls: the same bytes; rows = 0, decode = 1: the paths, scores and
    weights of the full call, no rows; rows = 1, decode = 0: its rows"""
    from wfsa_amd import _lib
    fsa, w, sym, off, p = M.expected("tiles200")[:5]
    first, _ = _run("tiles200", monkeypatch)
    dev = _device(fsa, sym, off, p, monkeypatch)
    _same_bytes(first, dev.dense_byte_marginals(w, rows=True, decode=True))
    alone = dev.dense_byte_marginals(w, rows=False, decode=True)
    _same_bytes(first[3:], alone[3:])
    assert len(alone[1]) == 0 and len(alone[2]) == 0
    mrow = np.zeros(off[-1] + 1, dtype=np.int64)
    assert _lib.load().wfsa_dev_dense_byte_marginals_get(dev._h, mrow.ctypes.data, None, None) == _lib.WFSA_ERR_ARG
    rows = dev.dense_byte_marginals(w, rows=True, decode=False)
    assert len(rows) == 5
    _same_bytes(first[:5], rows)
    prow = np.zeros(len(p) + 1, dtype=np.int64)
    assert _lib.load().wfsa_dev_dense_byte_marginals_path_get(dev._h, prow.ctypes.data, None) == _lib.WFSA_ERR_ARG
    _same_bytes(first, dev.dense_byte_marginals(w, rows=True, decode=True))


@pytest.mark.parametrize("name", ["holes12", "without_a_path"])
def test_strings_without_a_path(name, monkeypatch):
    """log q -inf, empty rows and paths, score NaN, weight -inf, with p > 0 and
    with p = 0 on those strings; the other strings' outputs (their neighbours
    in the slots among them) are the bytes of the p > 0 call and within the cap"""
    fsa, w, sym, off, p, tab, rlogq, rmass = M.expected(name)
    res, _ = _run(name, monkeypatch)
    mrow, midx, mval, boundary, logq, score, plw, prow, pidx = res
    none = np.isneginf(rlogq)
    assert none.any() and (~none).any()
    assert np.array_equal(np.isneginf(logq), none)
    for s in np.flatnonzero(none):
        assert mrow[off[s]] == mrow[off[s + 1]] and prow[s] == prow[s + 1]
        assert np.isnan(score[s]) and plw[s] == -np.inf
    assert np.isfinite(score[~none]).all() and np.isfinite(plw[~none]).all()
    assert np.isfinite(w[pidx]).all()
    p0 = np.where(none, 0.0, p)
    dev = _device(fsa, sym, off, p0 / p0.sum(), monkeypatch)
    again = dev.dense_byte_marginals(w, rows=True, decode=True)
    _same_bytes(res, again)
    _check_masses(name, again)


def test_results_survive_the_other_dense_calls(monkeypatch):
    from wfsa_amd import _lib
    lib = _lib.load()
    fsa, w, sym, off, p = M.expected("dense16")[:5]
    dev = _device(fsa, sym, off, p, monkeypatch)
    rng = np.random.default_rng(9)
    w2 = rng.normal(-1.0, 0.5, size=dev.n_params)
    res = dev.dense_byte_marginals(w, rows=True, decode=True)
    _same_bytes(res, _run("dense16", monkeypatch)[0])
    best = dev.dense_best_paths(w2)           # (both overwrite the shared history)
    samp = dev.dense_sample_paths(w2, 3, 1)
    mrow, midx, mval = np.zeros_like(res[0]), np.zeros_like(res[1]), np.zeros_like(res[2])
    assert lib.wfsa_dev_dense_byte_marginals_get(dev._h, mrow.ctypes.data, midx.ctypes.data, mval.ctypes.data) == 0
    _same_bytes(res[:3], (mrow, midx, mval))
    prow, pidx = np.zeros_like(res[7]), np.zeros_like(res[8])
    assert lib.wfsa_dev_dense_byte_marginals_path_get(dev._h, prow.ctypes.data, pidx.ctypes.data) == 0
    _same_bytes(res[7:], (prow, pidx))
    # and theirs survive a byte-marginals call
    dev.dense_byte_marginals(w, rows=True, decode=True)
    brow, bidx = np.zeros_like(best[1]), np.zeros(max(len(best[2]), 1), dtype=np.int32)
    assert lib.wfsa_dev_dense_best_paths_get(dev._h, brow.ctypes.data, bidx.ctypes.data) == 0
    assert brow.tobytes() == best[1].tobytes() and bidx[:len(best[2])].tobytes() == best[2].tobytes()
    srow, slogw = np.zeros_like(samp[0]), np.zeros_like(samp[1])
    sprow, spidx = np.zeros_like(samp[2]), np.zeros(max(len(samp[3]), 1), dtype=np.int32)
    assert lib.wfsa_dev_dense_sample_paths_get(dev._h, srow.ctypes.data, slogw.ctypes.data, sprow.ctypes.data, spidx.ctypes.data) == 0
    _same_bytes(samp[:3], (srow, slogw, sprow))
    assert spidx[:len(samp[3])].tobytes() == samp[3].tobytes()
    # the decoders after the call has used the shared history
    _same_bytes(best, dev.dense_best_paths(w2))
    _same_bytes(samp, dev.dense_sample_paths(w2, 3, 1))


def test_byte_marginals_leave_rmin_and_the_evaluations_alone(monkeypatch):
    fsa, w, sym, off, p = M.expected("dense16")[:5]
    dev = _device(fsa, sym, off, p, monkeypatch)
    dev.recognize()
    rng = np.random.default_rng(9)
    w1 = rng.normal(-1.0, 0.5, size=dev.n_params)
    w2 = rng.normal(-1.0, 0.5, size=dev.n_params)
    dev.objective_grad(w1, want_logq=False)
    plain = dev.rmin()
    assert plain[1] >= 0
    dev.objective_grad(w1, want_logq=False)
    dev.dense_byte_marginals(w2, rows=True, decode=True)
    assert dev.rmin() == plain
    ll, grad, logq = dev.objective_grad(w1)
    dev.dense_byte_marginals(w2, rows=True, decode=True)
    ll2, grad2, logq2 = dev.objective_grad(w1)
    assert ll == ll2 and grad.tobytes() == grad2.tobytes() and logq.tobytes() == logq2.tobytes()


def _qn_spec():
    return dict(n_states=16, degree=1, vocab=8, emissions=2, dense=True, n_strings=300, max_len=9, seed=21)


def test_byte_marginals_leave_the_quasinewton_loop_alone(monkeypatch):
    """Run(3), Run(3) gives info rows bit-equal to Run(3), ByteMarginals(True),
    Run(3) on a dense learner (rmin columns on)"""
    import wfsa_amd as W
    monkeypatch.setenv("WFSA_DENSE", "1")
    syn = W.Synthetic(**_qn_spec())
    sym, off, wt = syn.corpus()
    fsa = W.Fsa.read_text(syn.wfsa_text)
    runs = []
    for marg in (False, True):
        lrn = W.QuasiNewtonLearner(0)
        lrn.set_info_rmin(True)
        lrn.BuildFromPacked(fsa, sym, off, wt)
        lrn.Finalize()
        lrn.Init(7)
        assert lrn.stats()["dense"] == 1
        rows = lrn.Run(3, 1.0, -1.0)
        if marg:
            mrow, midx, mval, boundary, logq, score, plw, prow, pidx = lrn.ByteMarginals(True)
            assert len(logq) == len(wt) and np.isfinite(logq).all() and (boundary == 1.0).all()
            assert (np.diff(mrow) > 0).all() and (score > 0.0).all() and (np.diff(prow) > 0).all()
        rows += lrn.Run(3, 1.0, -1.0)
        runs.append(np.array(rows))
    assert runs[0].shape == (6, 7)
    assert runs[0].tobytes() == runs[1].tobytes()
    assert W.HessianLearner.ByteMarginals is W.QuasiNewtonLearner.ByteMarginals


def test_learner_byte_marginals_on_a_dense_model(monkeypatch):
    """QuasiNewtonLearner.ByteMarginals(decode=True) after a few steps equals
    Device.dense_byte_marginals at the learner's weights; boundary is 1.0; the
    state ids name states of Fsa.state_names()"""
    import wfsa_amd as W
    monkeypatch.setenv("WFSA_DENSE", "1")
    syn = W.Synthetic(**_qn_spec())
    sym, off, wt = syn.corpus()
    fsa = W.Fsa.read_text(syn.wfsa_text)
    lrn = W.QuasiNewtonLearner(0)
    lrn.BuildFromPacked(fsa, sym, off, wt)
    lrn.Finalize()
    lrn.Init(7)
    lrn.Run(3, 1.0, -1.0)
    assert lrn.stats()["dense"] == 1
    got = lrn.ByteMarginals(decode=True)
    assert len(got) == 9 and (got[3] == 1.0).all() and len(got[3]) == off[-1]
    plain = lrn.ByteMarginals()
    assert len(plain) == 5
    _same_bytes(got[:5], plain)
    tw = lrn.trimmed_index()
    w_dev = np.where(tw >= 0, np.append(lrn.x(), 0.0)[tw], np.where(tw == -1, 0.0, -np.inf))   # GetWeight
    dev = _device(fsa, sym, off, wt / wt.sum(), monkeypatch)
    _same_bytes(got, dev.dense_byte_marginals(w_dev, rows=True, decode=True))
    names = fsa.state_names()
    assert got[1].max() < len(names) and not {names[u] for u in got[1]} & {"^", "$"}


def test_cli_byte_marginal_files_on_a_dense_model(tmp_path, monkeypatch):
    """wfsa -bm FILE -md FILE on a dense model: the files parse to the values
    of the Python learner taking the same steps"""
    import wfsa_amd as W
    syn = W.Synthetic(**dict(R.BYTE_CASES["dense16"][0], seed=21))
    sym, off, wt = syn.corpus()
    model, corpus = str(tmp_path / "dense16.wfsa"), str(tmp_path / "dense16.corpus")
    open(model, "wb").write(syn.wfsa_text.encode("latin-1"))
    with open(corpus, "wb") as f:
        f.write(b"\n")
        for i in range(len(wt)):
            f.write(bytes(sym[off[i]:off[i + 1]]) + b" %d\n" % int(wt[i]))
    bm, md = str(tmp_path / "bm.tsv"), str(tmp_path / "md.tsv")
    r = subprocess.run([CLI, "-a", model, "-c", corpus, "-opt", "QuasiNewton", "-e", "3", "-i", "1", "-s", "-bm", bm, "-md", md],
                       capture_output=True, text=True, timeout=120, env=dict(os.environ, WFSA_DENSE="1"))
    assert r.returncode == 0, r.stderr[-2000:]

    monkeypatch.setenv("WFSA_DENSE", "1")
    crp = W.Corpus.read_file(corpus)
    fsa = W.Fsa.read_file(model)
    lrn = W.QuasiNewtonLearner(0)
    lrn.BuildFrom(fsa, crp)
    lrn.Finalize()
    lrn.Init(1)
    for _ in range(3):   # the CLI's epoch loop: eta 1, tol 1e-6
        _, halt = lrn.OptimizationStep(1.0, 1e-6)
        if halt:
            break
    assert lrn.stats()["dense"] == 1
    mrow, midx, mval, boundary, logq, score, plw, prow, pidx = lrn.ByteMarginals(True)
    names = fsa.state_names()
    strings, _ = crp.strings()
    _, rec = lrn.path_counts()
    want = [s for s, k in zip(strings, rec) if k]
    assert len(want) > 0 and len(logq) == len(want) and len(boundary) == sum(len(s) for s in want)

    lines = open(bm, encoding="latin-1").read().split("\n")
    assert lines[-1] == ""
    rows = [l.split("\t") for l in lines[:-1]]
    assert [row[0] for row in rows] == want
    b = 0
    for s, row in enumerate(rows):
        assert float(row[1]) == logq[s] and len(row) == 2 + 2 * len(want[s])   # %.17g round-trips a double
        for i in range(len(want[s])):
            assert float(row[2 + 2 * i]) == boundary[b] == 1.0
            pairs = [q.rsplit(":", 1) for q in row[3 + 2 * i].split(",")]
            assert [q[0] for q in pairs] == [names[u] for u in midx[mrow[b]:mrow[b + 1]]] and len(pairs) > 0
            assert [float(q[1]) for q in pairs] == list(mval[mrow[b]:mrow[b + 1]])
            b += 1
    assert b == len(boundary)
    lines = open(md, encoding="latin-1").read().split("\n")
    assert lines[-1] == ""
    rows = [l.split("\t") for l in lines[:-1]]
    assert [row[0] for row in rows] == want
    for s, row in enumerate(rows):
        assert float(row[1]) == score[s] and 0.0 < score[s] <= len(want[s]) * (1.0 + 1e-9)
        assert abs(float(row[2]) - plw[s]) <= 1e-14 * max(1.0, abs(plw[s]))   # %.15g
        assert [int(v) for v in row[3].split()] == list(pidx[prow[s]:prow[s + 1]])


def test_dense_byte_marginals_errors(monkeypatch):
    import wfsa_amd as W
    from wfsa_amd import _lib
    lib = _lib.load()
    fsa, w0, sym, off, p = M.expected("dense16")[:5]

    def arg_error(dev, w, word, rows=True, decode=True):
        with pytest.raises(W.WfsaError) as e:
            dev.dense_byte_marginals(w, rows=rows, decode=decode)
        assert e.value.code == _lib.WFSA_ERR_ARG and word in str(e.value), str(e.value)

    def get_rc(dev):
        mrow = np.zeros(off[-1] + 1, dtype=np.int64)
        prow = np.zeros(len(p) + 1, dtype=np.int64)
        return (lib.wfsa_dev_dense_byte_marginals_get(dev._h, mrow.ctypes.data, None, None),
                lib.wfsa_dev_dense_byte_marginals_path_get(dev._h, prow.ctypes.data, None))

    monkeypatch.setenv("WFSA_DENSE", "1")
    dev = W.Device(0)
    arg_error(dev, np.zeros(0), "load a model")              # nothing loaded
    dev.load_model(fsa)
    arg_error(dev, np.zeros(dev.n_params), "load a model")   # no corpus
    dev.load_corpus(sym, off, p)
    assert dev.stats()["dense"] == 1
    assert get_rc(dev) == (_lib.WFSA_ERR_ARG, _lib.WFSA_ERR_ARG)   # without a result since the load
    w = np.full(dev.n_params, -1.0)
    arg_error(dev, w, "ask for nothing", rows=False, decode=False)
    for bad in (np.nan, np.inf):                             # a NaN or +inf weight (-inf is allowed)
        wb = w.copy()
        wb[dev.n_params // 2] = bad
        arg_error(dev, wb, "NaN or +inf")
    dev.recognize()
    dev.objective_grad_begin(w)                              # while an evaluation is in flight
    arg_error(dev, w, "in flight")
    dev.objective_grad_end()
    res = dev.dense_byte_marginals(w, rows=True, decode=True)
    assert np.isfinite(res[5]).all() and get_rc(dev) == (0, 0)
    dev.dense_byte_marginals(w, rows=False, decode=True)     # _get after rows = 0
    assert get_rc(dev) == (_lib.WFSA_ERR_ARG, 0)
    dev.dense_byte_marginals(w, rows=True, decode=False)     # _path_get after decode = 0
    assert get_rc(dev) == (0, _lib.WFSA_ERR_ARG)
    dev.load_corpus(sym, off, p)                             # a load ends the result
    assert get_rc(dev) == (_lib.WFSA_ERR_ARG, _lib.WFSA_ERR_ARG)
    with pytest.raises(W.WfsaError) as e:                    # the trellis entry point keeps its contract
        dev.byte_marginals(w)
    assert e.value.code == _lib.WFSA_ERR_CAPACITY and "WFSA_DENSE=0" in str(e.value)
    dev.load_paths(2, [0, 1, 2], [0, 1], [1.0, 1.0], [0, 2], [0, 1], [1.0])   # matrix-file mode: no automaton
    arg_error(dev, np.zeros(2), "matrix")
    tr = _device(fsa, sym, off, p, monkeypatch, dense=False)   # not on the dense path: the other entry point serves it
    arg_error(tr, w, "wfsa_dev_byte_marginals")
    assert len(tr.byte_marginals(w)[1]) > 0


def test_dense_byte_marginals_stats(monkeypatch):
    fsa, w, sym, off, p = M.expected("dense16")[:5]
    dev = _device(fsa, sym, off, p, monkeypatch)
    dev.dense_byte_marginals(w, rows=True, decode=True)
    st = dev.stats()
    parts = [st[k] for k in ("dense_bm_forward_ms", "dense_bm_backward_ms", "dense_bm_rows_ms", "dense_bm_decode_ms")]
    assert all(v > 0.0 for v in parts) and st["byte_marginal_ms"] > 0.0
    assert abs(sum(parts) - st["byte_marginal_ms"]) <= 1e-9 * st["byte_marginal_ms"]
    dev.dense_byte_marginals(w, rows=False, decode=True)
    st = dev.stats()
    assert st["dense_bm_rows_ms"] == 0.0 and st["dense_bm_decode_ms"] > 0.0
