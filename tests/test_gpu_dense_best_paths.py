"""GPU tests of the Viterbi decode on the dense path
(wfsa_dev_dense_best_paths, dense_decode.hip): the (max, +) pass over the row
slots and its back-track, against the oracle's enumerated paths, against the
trellis decode of the same model loaded with WFSA_DENSE=0 (byte for byte, for
the cases whose decisions test_dense_decode_reference.py found wider than
1e-9), and against the numpy restatement (dense_decode_reference.py) bit for
bit.  Needs a gfx950 device."""
import os
import subprocess

import numpy as np
import pytest

import dense_decode_reference as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "w-fsa_amd", "wfsa_amd", "wfsa")
DENSE16 = R.BYTE_CASES["dense16"][0]
# Learned weights carry exact ties: parameters that share a value give different paths the same weight, most strings
# have several maximisers, and where their sums round differently in the two decoders ((D + lA) + lE here, D + (lA + lE)
# in the trellis decode) each may return another one of them -- at equal weight.  Comparing PATHS after learning is
# therefore a fair demand only where the two tie-breaks coincide; these corpus seeds are such cases (of the seeds tried,
# about one in three for either flow), found by running both decoders, not by loosening the comparison.
LEARN16 = dict(DENSE16, seed=1)
CLI16 = dict(DENSE16, seed=21)


def _device(fsa, sym, off, wt, monkeypatch, dense):
    """dense: True forced, False the trellis tiers, None chosen by the library"""
    import wfsa_amd as W
    if dense is None:
        monkeypatch.delenv("WFSA_DENSE", raising=False)
    else:
        monkeypatch.setenv("WFSA_DENSE", "1" if dense else "0")
    dev = W.Device(0)
    dev.load_model(fsa)
    dev.load_corpus(sym, off, wt / wt.sum())
    if dense is not None:
        assert dev.stats()["dense"] == (1 if dense else 0)
    return dev


def _same_bytes(a, b):
    for u, v in zip(a, b):
        assert u.dtype == v.dtype and u.shape == v.shape
        assert u.tobytes() == v.tobytes()


def _equals_reference(got, fsa, w, sym, off):
    """every string's logw bit-equal to the numpy restatement's, ids equal"""
    logw, prow, pidx = got
    rl, rp, ri, _, _ = R.decode_corpus(fsa, w, sym, off)
    assert logw.tobytes() == rl.tobytes(), np.flatnonzero(logw != rl)[:5]
    np.testing.assert_array_equal(prow, rp)
    np.testing.assert_array_equal(pidx, ri)
    return rl


def test_dense_best_paths_against_the_oracles_enumerated_paths(monkeypatch):
    """the rmin enumeration case (5 states forced dense: one tile, mostly
    padded states), three weight draws, test_gpu_best_paths' acceptance rule"""
    import wfsa_amd as W
    from decode_cases import _reference
    from test_gpu_best_paths import _accept
    syn = W.Synthetic(n_states=5, degree=1, vocab=3, emissions=2, dense=True, n_strings=60, max_len=5, seed=9)
    sym, off, wt = syn.corpus()
    ref = _reference(syn.wfsa_text, sym, off, wt)
    fsa = W.Fsa.read_text(syn.wfsa_text)
    dev = _device(fsa, sym, off, wt, monkeypatch, dense=True)
    o = ref["o"]
    names = {n: j for j, n in enumerate(o.full_param_names())}
    perm = np.array([names[n] for n in fsa.param_names()], dtype=np.int64)
    n_all = len(off) - 1
    assert len(ref["rec"]) == n_all
    rng = np.random.default_rng(7)
    for _ in range(3):
        x = rng.normal(-1.0, 0.5, size=o.n)
        o.set_x(x)
        w = o.w_full()[perm]
        logw, prow, pidx = dev.dense_best_paths(w)
        assert logw.shape == (n_all,) and prow.shape == (n_all + 1,) and prow[0] == 0 and prow[-1] == len(pidx)
        _accept(ref, x, perm, w, logw, prow, pidx, ref["rec"])


@pytest.mark.parametrize("name", ["dense16", "auto128"])
def test_dense_best_paths_equal_the_trellis_decode_byte_for_byte(name, monkeypatch):
    """logw, prow and pidx equal Device.best_paths of the same model loaded
    with WFSA_DENSE=0; auto128 takes the dense path without being forced"""
    import wfsa_amd as W
    text, sym, off, wt = R.synthetic(name)
    fsa = W.Fsa.read_text(text)
    w = R.case_weights(name, len(fsa.param_names()))
    dn = _device(fsa, sym, off, wt, monkeypatch, dense=None if name == "auto128" else True)
    assert dn.stats()["dense"] == 1
    got = dn.dense_best_paths(w)
    sp = _device(fsa, sym, off, wt, monkeypatch, dense=False)
    _same_bytes(got, sp.best_paths(w))
    assert np.isfinite(got[0]).all()


def test_dense_best_paths_tiles_and_slots_against_numpy(monkeypatch):
    """200 states (np 256: two column tiles, 16 K slices, padded states) and
    64 states with several strings per slot: start rows mid-column, two row
    tiles; every string's logw bit-equal to the restatement's, ids equal"""
    import wfsa_amd as W
    packed = tiles = False
    for spec, seed in ((dict(n_states=200, vocab=5, emissions=2, n_strings=300, max_len=40, seed=12), 8),
                       (dict(n_states=64, vocab=8, emissions=3, n_strings=600, max_len=12, seed=13), 9)):
        syn = W.Synthetic(degree=1, dense=True, **spec)
        sym, off, wt = syn.corpus()
        fsa = W.Fsa.read_text(syn.wfsa_text)
        w = np.random.default_rng(seed).normal(-1.0, 0.5, size=len(fsa.param_names()))
        dev = _device(fsa, sym, off, wt, monkeypatch, dense=True)
        st = dev.stats()
        packed |= len(wt) > st["dense_rows"]
        tiles |= st["dense_rows"] >= 256
        if spec["n_states"] == 200:
            assert st["dense_np"] == 256
        rl = _equals_reference(dev.dense_best_paths(w), fsa, w, sym, off)
        assert np.isfinite(rl).all()
    assert packed and tiles


def test_dense_best_paths_ties_go_to_the_lowest_state(monkeypatch):
    """all-zero weights on the 16-state model: every decision is an exact tie.
    The result equals the restatement's (np.argmax: the lowest state) and the
    trellis decode's: for a model that qualifies for the dense path the
    trellis tier lists a node's in-edges by ascending source state (one edge
    per source, byte and destination), so its first in-edge, lowest end node
    and first end edge are the lowest states too."""
    import wfsa_amd as W
    text, sym, off, wt = R.synthetic("dense16")
    fsa = W.Fsa.read_text(text)
    w = np.zeros(len(fsa.param_names()))
    dn = _device(fsa, sym, off, wt, monkeypatch, dense=True)
    got = dn.dense_best_paths(w)
    _equals_reference(got, fsa, w, sym, off)
    sp = _device(fsa, sym, off, wt, monkeypatch, dense=False)
    _same_bytes(got, sp.best_paths(w))


def test_dense_best_paths_without_a_path(monkeypatch):
    """the most-used quarter of the parameters at -inf, the corpus extended by
    an empty string and by a string with a byte no state emits: -inf and empty
    ranges exactly where the restatement has them, the empty string by the
    ^ -> $ rule, no returned path across a -inf parameter"""
    import wfsa_amd as W
    text, sym, off, wt = R.synthetic("dense16")
    fsa = W.Fsa.read_text(text)
    n_par = len(fsa.param_names())
    w = R.case_weights("dense16", n_par)
    _, _, pidx0, _, _ = R.decode_corpus(fsa, w, sym, off)
    used = np.bincount(pidx0, minlength=n_par)
    w[np.argsort(-used, kind="stable")[:n_par // 4]] = -np.inf
    strings = [bytes(sym[off[i]:off[i + 1]]) for i in range(len(wt))]
    strings += [b"", strings[0][:1] + b"\xff" + strings[0][1:]]
    sym2 = np.frombuffer(b"".join(strings), dtype=np.uint8).copy()
    off2 = np.concatenate([[0], np.cumsum([len(s) for s in strings])]).astype(np.int64)
    wt2 = np.concatenate([wt, [1.0, 1.0]])
    dev = _device(fsa, sym2, off2, wt2, monkeypatch, dense=True)
    logw, prow, pidx = got = dev.dense_best_paths(w)
    rl = _equals_reference(got, fsa, w, sym2, off2)
    none = np.isneginf(rl)
    assert none[-1] and none.any() and (~none).any()
    assert (np.diff(prow)[none] == 0).all() and (np.diff(prow)[~none] > 0).all()
    tab = R.Tables(fsa, w)
    empty = len(strings) - 2
    if tab.pse == -2 or not tab.lse > -np.inf:   # no ^ -> $ edge (or at -inf): no path
        assert logw[empty] == -np.inf and prow[empty] == prow[empty + 1]
    else:                                        # that edge alone
        assert logw[empty] == tab.lse and list(pidx[prow[empty]:prow[empty + 1]]) == [p for p in [tab.pse] if p >= 0]
    assert np.isfinite(w[pidx]).all()


def test_dense_best_paths_repeat_byte_for_byte(monkeypatch):
    import wfsa_amd as W
    text, sym, off, wt = R.synthetic("dense16")
    fsa = W.Fsa.read_text(text)
    w = R.case_weights("dense16", len(fsa.param_names()))
    dev = _device(fsa, sym, off, wt, monkeypatch, dense=True)
    first = dev.dense_best_paths(w)
    second = dev.dense_best_paths(w)
    _same_bytes(first, second)
    st = dev.stats()
    assert st["best_path_ms"] > 0.0
    parts = st["dense_bp_tables_ms"] + st["dense_bp_forward_ms"] + st["dense_bp_backtrack_ms"]
    assert abs(parts - st["best_path_ms"]) <= 1e-9 * st["best_path_ms"]


def _qn_spec():
    return dict(n_states=16, degree=1, vocab=8, emissions=2, dense=True, n_strings=300, max_len=9, seed=21)


def test_dense_decoder_leaves_the_quasinewton_loop_alone(monkeypatch):
    """Run(3), Run(3) gives info rows bit-equal to Run(3), BestPaths(), Run(3)
    on a dense learner (rmin columns on)"""
    import wfsa_amd as W
    monkeypatch.setenv("WFSA_DENSE", "1")
    syn = W.Synthetic(**_qn_spec())
    sym, off, wt = syn.corpus()
    fsa = W.Fsa.read_text(syn.wfsa_text)
    runs = []
    for decode in (False, True):
        lrn = W.QuasiNewtonLearner(0)
        lrn.set_info_rmin(True)
        lrn.BuildFromPacked(fsa, sym, off, wt)
        lrn.Finalize()
        lrn.Init(7)
        assert lrn.stats()["dense"] == 1
        rows = lrn.Run(3, 1.0, -1.0)
        if decode:
            logw, prow, pidx = lrn.BestPaths()
            assert np.isfinite(logw).all() and (np.diff(prow) > 0).all()
        rows += lrn.Run(3, 1.0, -1.0)
        runs.append(np.array(rows))
    assert runs[0].shape == (6, 7)
    assert runs[0].tobytes() == runs[1].tobytes()


def test_dense_decoder_leaves_rmin_alone(monkeypatch):
    """rmin() after an evaluation is unchanged by a dense_best_paths call at
    other weights in between"""
    import wfsa_amd as W
    text, sym, off, wt = R.synthetic("dense16")
    fsa = W.Fsa.read_text(text)
    dev = _device(fsa, sym, off, wt, monkeypatch, dense=True)
    dev.recognize()
    rng = np.random.default_rng(9)
    w1 = rng.normal(-1.0, 0.5, size=dev.n_params)
    w2 = rng.normal(-1.0, 0.5, size=dev.n_params)
    dev.objective_grad(w1, want_logq=False)
    plain = dev.rmin()
    assert plain[1] >= 0
    dev.objective_grad(w1, want_logq=False)
    dev.dense_best_paths(w2)
    assert dev.rmin() == plain


def test_learner_best_paths_on_a_dense_model(monkeypatch):
    """QuasiNewtonLearner.BestPaths() after run(flags=7, epochs=4): the dense
    learner's paths equal those of the same learner under WFSA_DENSE=0, given
    close final x; logw within 1e-10 (the two learning paths round differently).
    At the dense learner's weights no decision between DISTINCT values on a
    returned path is closer than 1e-6 (the restatement's gaps), so the 1e-9
    between the two x cannot turn one; see LEARN16 for the exact ties"""
    import wfsa_amd as W
    syn = W.Synthetic(**LEARN16)
    sym, off, wt = syn.corpus()
    fsa = W.Fsa.read_text(syn.wfsa_text)
    res = {}
    for dense in (True, False):
        monkeypatch.setenv("WFSA_DENSE", "1" if dense else "0")
        lrn = W.QuasiNewtonLearner(0)
        lrn.BuildFromPacked(fsa, sym, off, wt)
        lrn.Finalize()
        rows = lrn.run(flags=7, epochs=4)
        assert len(rows) == 4 and lrn.stats()["dense"] == (1 if dense else 0)
        res[dense] = (lrn.x(),) + tuple(lrn.BestPaths())
        if dense:
            tw = lrn.trimmed_index()
            w_dev = np.where(tw >= 0, np.append(lrn.x(), 0.0)[tw], np.where(tw == -1, 0.0, -np.inf))   # GetWeight
            rl, rp, ri, gaps, _ = R.decode_corpus(fsa, w_dev, sym, off)
            print("smallest on-path gap between distinct values", gaps.min())
            assert gaps.min() > 1e-6
            assert res[True][1].tobytes() == rl.tobytes()
            np.testing.assert_array_equal(res[True][3], ri)
    np.testing.assert_allclose(res[True][0], res[False][0], rtol=1e-9, atol=1e-11)
    np.testing.assert_array_equal(res[True][2], res[False][2])
    np.testing.assert_array_equal(res[True][3], res[False][3])
    assert np.isfinite(res[True][1]).all() and len(res[True][1]) == len(wt)
    assert (np.abs(res[True][1] - res[False][1]) <= 1e-10 * np.maximum(1.0, np.abs(res[False][1]))).all()
    assert W.HessianLearner.BestPaths is W.QuasiNewtonLearner.BestPaths


def test_cli_best_paths_file_on_a_dense_model(tmp_path):
    """wfsa -bp FILE on a dense model: the strings and the path columns equal
    the WFSA_DENSE=0 run's, the log weights agree within 1e-10 (CLI16: a corpus
    on which the two decoders break the learned weights' exact ties alike)"""
    import wfsa_amd as W
    syn = W.Synthetic(**CLI16)
    sym, off, wt = syn.corpus()
    model, corpus = str(tmp_path / "dense16.wfsa"), str(tmp_path / "dense16.corpus")
    open(model, "wb").write(syn.wfsa_text.encode("latin-1"))
    with open(corpus, "wb") as f:
        f.write(b"\n")
        for i in range(len(wt)):
            f.write(bytes(sym[off[i]:off[i + 1]]) + b" %d\n" % int(wt[i]))
    rows = {}
    for dense in ("1", "0"):
        out = str(tmp_path / ("best%s.tsv" % dense))
        r = subprocess.run([CLI, "-a", model, "-c", corpus, "-opt", "QuasiNewton", "-e", "3", "-i", "1", "-s", "-bp", out],
                           capture_output=True, text=True, timeout=120, env=dict(os.environ, WFSA_DENSE=dense))
        assert r.returncode == 0, r.stderr[-2000:]
        lines = open(out, encoding="latin-1").read().split("\n")
        assert lines[-1] == ""
        rows[dense] = [l.split("\t") for l in lines[:-1]]
        assert len(rows[dense]) > 0 and all(len(row) == 4 for row in rows[dense])
    assert [row[0] for row in rows["1"]] == [row[0] for row in rows["0"]]
    assert [row[3] for row in rows["1"]] == [row[3] for row in rows["0"]]
    for a, b in zip(rows["1"], rows["0"]):
        assert len(a[3].split()) > 0
        assert abs(float(a[1]) - float(b[1])) <= 1e-10 * max(1.0, abs(float(b[1])))


def test_dense_best_paths_errors(monkeypatch):
    import wfsa_amd as W
    from wfsa_amd import _lib
    text, sym, off, wt = R.synthetic("dense16")
    fsa = W.Fsa.read_text(text)

    def arg_error(dev, w, word):
        with pytest.raises(W.WfsaError) as e:
            dev.dense_best_paths(w)
        assert e.value.code == _lib.WFSA_ERR_ARG and word in str(e.value), str(e.value)

    monkeypatch.setenv("WFSA_DENSE", "1")
    dev = W.Device(0)
    arg_error(dev, np.zeros(0), "load a model")          # nothing loaded
    dev.load_model(fsa)
    arg_error(dev, np.zeros(dev.n_params), "load a model")   # no corpus
    dev.load_corpus(sym, off, wt / wt.sum())
    assert dev.stats()["dense"] == 1
    # _get without a result since the load
    prow = np.zeros(len(wt) + 1, dtype=np.int64)
    rc = _lib.load().wfsa_dev_dense_best_paths_get(dev._h, prow.ctypes.data, None)
    assert rc == _lib.WFSA_ERR_ARG
    w = np.full(dev.n_params, -1.0)
    # a NaN or +inf weight (-inf is allowed)
    for bad in (np.nan, np.inf):
        wb = w.copy()
        wb[dev.n_params // 2] = bad
        arg_error(dev, wb, "NaN or +inf")
    # while an evaluation is in flight
    dev.recognize()
    dev.objective_grad_begin(w)
    arg_error(dev, w, "in flight")
    dev.objective_grad_end()
    logw, prow, pidx = dev.dense_best_paths(w)
    assert np.isfinite(logw).all()
    # a load ends the result
    dev.load_corpus(sym, off, wt / wt.sum())
    assert _lib.load().wfsa_dev_dense_best_paths_get(dev._h, prow.ctypes.data, None) == _lib.WFSA_ERR_ARG
    # the trellis entry point keeps its contract on the dense path
    with pytest.raises(W.WfsaError) as e:
        dev.best_paths(w)
    assert e.value.code == _lib.WFSA_ERR_CAPACITY and "WFSA_DENSE=0" in str(e.value)
    # matrix-file mode: no automaton
    dev.load_paths(2, [0, 1, 2], [0, 1], [1.0, 1.0], [0, 2], [0, 1], [1.0])
    arg_error(dev, np.zeros(2), "matrix")
    # a context that is not on the dense path: the other entry point serves it
    sp = _device(fsa, sym, off, wt, monkeypatch, dense=False)
    arg_error(sp, w, "wfsa_dev_best_paths")
    assert np.isfinite(sp.best_paths(w)[0]).all()
