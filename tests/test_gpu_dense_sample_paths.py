"""GPU tests of posterior path sampling on the dense path
(wfsa_dev_dense_sample_paths, dense_sample.hip): forward filter / backward
sample over the row slots, against the numpy restatement
(dense_sample_reference.py) sample by sample, against the trellis sampler of
the same model loaded with WFSA_DENSE=0, log q byte for byte against
objective_grad, on the hand-built gadgets of dense_gadgets.py, and through the
learner and the CLI.  A sample is compared path for path unless the
restatement found one of its choices closer than 1e-9 to a running-sum
boundary (test_dense_sample_reference.py: under 1% of each case).  Needs a
gfx950 device."""
import os
import subprocess

import numpy as np
import pytest

import dense_decode_reference as R
import dense_sample_reference as D
from conftest import ROOT

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "w-fsa_amd", "wfsa_amd", "wfsa")
LOGQ_REL = 1e-12   # test_gpu_dense.py's bound on log q against its reference


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
    for u, v in zip(a, b):
        assert u.dtype == v.dtype and u.shape == v.shape
        assert u.tobytes() == v.tobytes()


def _paths_equal(got, want, margin, what):
    """srow equal; every sample with margin >= 1e-9 has want's ids and want's
    logw to the bit; at most 1% of the samples are exempt"""
    srow, logw, prow, pidx = got[:4]
    wrow, wlogw, wprow, widx = want[:4]
    np.testing.assert_array_equal(srow, wrow)
    assert len(logw) == len(wlogw) == len(margin) and len(prow) == len(logw) + 1 and prow[-1] == len(pidx)
    exempt = margin < D.MARGIN
    differ = 0
    for t in np.flatnonzero(~exempt):
        assert np.array_equal(pidx[prow[t]:prow[t + 1]], widx[wprow[t]:wprow[t + 1]]), (what, t, margin[t])
        assert logw[t:t + 1].tobytes() == wlogw[t:t + 1].tobytes(), (what, t, logw[t], wlogw[t])
    for t in np.flatnonzero(exempt):
        differ += not np.array_equal(pidx[prow[t]:prow[t + 1]], widx[wprow[t]:wprow[t + 1]])
    print(f"dense_sample_paths | {what} | samples {len(margin)} exempt {int(exempt.sum())} of them different {differ}")
    assert exempt.mean() <= D.EXEMPT


def _logq_close(got, want):
    none = np.isneginf(want)
    assert np.array_equal(np.isneginf(got), none)
    np.testing.assert_allclose(got[~none], want[~none], rtol=LOGQ_REL)


def _against_restatement(name, monkeypatch, dense=True, n=D.N_PATHS):
    fsa, w, sym, off, p = D.case(name)
    dev = _device(fsa, sym, off, p, monkeypatch, dense)
    got = dev.dense_sample_paths(w, n, D.SEED)
    want = D.expected(name, n)
    _paths_equal(got, want, want[5], name)
    _logq_close(got[4], want[4])
    return dev, got, want, (fsa, w, sym, off, p)


@pytest.mark.parametrize("name", ["dense16", "auto128", "tiles200", "slots64"])
def test_dense_sample_paths_equal_the_restatement_sample_by_sample(name, monkeypatch):
    """n = 5; tiles200: np = 256 -- four groups of 64, two column tiles, padded
    states, several strings per slot; slots64: several row tiles"""
    dev, got, want, (fsa, w, sym, off, p) = _against_restatement(name, monkeypatch, dense=None if name == "auto128" else True)
    st = dev.stats()
    assert (np.diff(got[0]) == D.N_PATHS).all() and np.isfinite(got[4]).all()
    if name == "tiles200":   # (and several strings per row slot: a start row mid-column)
        assert st["dense_np"] == 256 and len(p) > st["dense_rows"]
    if name == "slots64":    # (several row tiles)
        assert st["dense_rows"] >= 256
    assert (got[1] - np.repeat(got[4], D.N_PATHS) <= 1e-12 * np.abs(np.repeat(got[4], D.N_PATHS))).all()


@pytest.mark.parametrize("name", ["dense16", "auto128"])
def test_dense_sample_paths_equal_the_trellis_sampler(name, monkeypatch):
    """the same uniforms and candidate order: srow equal, and every sample the
    restatement does not exempt has the trellis sampler's ids and logw bytes"""
    fsa, w, sym, off, p = D.case(name)
    dn = _device(fsa, sym, off, p, monkeypatch, dense=None if name == "auto128" else True)
    got = dn.dense_sample_paths(w, D.N_TRELLIS, D.SEED)
    sp = _device(fsa, sym, off, p, monkeypatch, dense=False)
    want = sp.sample_paths(w, D.N_TRELLIS, D.SEED)
    _paths_equal(got, want, D.expected(name, D.N_TRELLIS)[5], name + " vs trellis")
    np.testing.assert_allclose(got[4], want[4], rtol=LOGQ_REL)


def test_dense_sample_paths_logq_is_objective_grads_byte_for_byte(monkeypatch):
    """on a context running the default engine"""
    monkeypatch.delenv("WFSA_DENSE_ENGINE", raising=False)
    monkeypatch.delenv("WFSA_DENSE_BLAS", raising=False)
    for name in ("dense16", "tiles200"):
        fsa, w, sym, off, p = D.case(name)
        dev = _device(fsa, sym, off, p, monkeypatch)
        dev.recognize()
        _, _, logq = dev.objective_grad(w, want_logq=True)
        got = dev.dense_sample_paths(w, 2, 3)
        assert got[4].tobytes() == np.asarray(logq, dtype=np.float64).tobytes()
        # and before any evaluation has run on the context
        fresh = _device(fsa, sym, off, p, monkeypatch)
        assert fresh.dense_sample_paths(w, 2, 3)[4].tobytes() == got[4].tobytes()


@pytest.mark.parametrize("engine", ["fused", "blas", "dma"])
def test_dense_sample_paths_run_the_same_flow_on_every_engine(engine, monkeypatch):
    """whatever GEMM engine the context's evaluations run, the sampler runs the
    split-K flow: the bytes of a default-engine context (two column tiles)"""
    fsa, w, sym, off, p = D.case("edge129")
    monkeypatch.delenv("WFSA_DENSE_BLAS", raising=False)
    monkeypatch.delenv("WFSA_DENSE_ENGINE", raising=False)
    want = _device(fsa, sym, off, p, monkeypatch).dense_sample_paths(w, 3, 4)
    monkeypatch.setenv("WFSA_DENSE_ENGINE", engine)
    dev = _device(fsa, sym, off, p, monkeypatch)
    assert dev.stats()["dense_blas"] != 2   # (not the split-K engine)
    dev.recognize()
    dev.objective_grad(w)   # (the engine's own buffers in use)
    _same_bytes(want, dev.dense_sample_paths(w, 3, 4))


def test_dense_sample_paths_repeat_and_prefix(monkeypatch):
    """two calls: the same bytes; the first 5 samples of every string in an
    n = 64 result are the n = 5 result; n = 1; another seed: another result"""
    fsa, w, sym, off, p = D.case("dense16")
    dev = _device(fsa, sym, off, p, monkeypatch)
    five = dev.dense_sample_paths(w, 5, D.SEED)
    _same_bytes(five, dev.dense_sample_paths(w, 5, D.SEED))
    full = dev.dense_sample_paths(w, 64, D.SEED)
    S = len(p)
    assert (np.diff(full[0]) == 64).all()
    assert full[4].tobytes() == five[4].tobytes()
    for s in range(S):
        a, b = five[0][s], full[0][s]
        assert five[1][a:a + 5].tobytes() == full[1][b:b + 5].tobytes()
        assert five[3][five[2][a]:five[2][a + 5]].tobytes() == full[3][full[2][b]:full[2][b + 5]].tobytes()
        assert np.array_equal(np.diff(five[2][a:a + 6]), np.diff(full[2][b:b + 6]))
    _same_bytes(five, dev.dense_sample_paths(w, 5, D.SEED))   # (after the larger call's buffers)
    one = dev.dense_sample_paths(w, 1, D.SEED)
    assert (np.diff(one[0]) == 1).all()
    assert one[1].tobytes() == five[1][::5].tobytes()
    other = dev.dense_sample_paths(w, 5, D.SEED + 1)
    assert other[3].tobytes() != five[3].tobytes() and other[4].tobytes() == five[4].tobytes()


def test_gadget_holes12(monkeypatch):
    """absent edges, single-member groups, ^ -> $, the empty string, strings
    that die: paths and -inf exactly where the gadget's reference has them"""
    import dense_gadgets as G
    dev, got, want, (fsa, w, sym, off, p) = _against_restatement("holes12", monkeypatch)
    g = G.holes12()
    ref = G.reference(fsa, w, sym, off, p)
    srow, logw, prow, pidx, logq = got
    live = np.isfinite(np.asarray(ref.logq, dtype=np.float64))
    assert np.array_equal(np.isfinite(logq), live)
    assert np.array_equal(np.diff(srow), np.where(live, D.N_PATHS, 0))
    assert not live[g.notes["dead"]].any() and live[g.notes["empty"]]
    assert G.close(logq, ref.logq, G.LOGQ_REL)
    tab = R.Tables(fsa, w)
    e = g.notes["empty"]
    for t in range(srow[e], srow[e + 1]):   # n copies of the ^ -> $ edge
        assert logw[t] == tab.lse and list(pidx[prow[t]:prow[t + 1]]) == [q for q in [tab.pse] if q >= 0]
    assert np.isfinite(w[pidx]).all()
    assert (tab.pA == -1).any() or (tab.pE == -1).any() or (tab.p0 == -1).any() or (tab.pend == -1).any()


@pytest.mark.parametrize("name", ["seams", "edge129"])
def test_gadget_seams_and_tile_edge(name, monkeypatch):
    """seams: runs of length-1 strings in one slot; edge129: states either
    side of a column-tile edge (np = 256)"""
    dev, got, want, _ = _against_restatement(name, monkeypatch)
    assert (np.diff(got[0]) == D.N_PATHS).all()
    if name == "edge129":
        assert dev.stats()["dense_np"] == 256


def test_gadget_peaked(monkeypatch):
    """a 4e-18 alternative is never drawn in 64 samples: every sample is the
    dominant path"""
    import dense_gadgets as G
    dev, got, want, (fsa, w, sym, off, p) = _against_restatement("peaked", monkeypatch)
    g = G.peaked()
    names = [tuple(nm) for nm in fsa.param_names()]
    rare = [names.index(tuple(nm)) for nm in g.notes["rare"]]   # s0 -> s2 and what only that route uses
    assert w[rare[0]] == -0.5 - G.PEAKED_GAP
    srow, logw, prow, pidx, logq = dev.dense_sample_paths(w, 64, 77)
    assert (np.diff(srow) == 64).all()
    best_logw, brow, bidx = dev.dense_best_paths(w)
    assert not np.isin(pidx, rare).any()
    s = 1   # "ab" has two paths, over s1 and over s2: every sample is the dominant one
    assert g.notes["strings"][s] == "ab"
    for t in range(srow[s], srow[s + 1]):
        assert np.array_equal(pidx[prow[t]:prow[t + 1]], bidx[brow[s]:brow[s + 1]]) and logw[t] == best_logw[s]


def test_gadget_long300(monkeypatch):
    """log q near -12000: every sample finite, exp(logw - logq) <= 1"""
    dev, got, want, _ = _against_restatement("long300", monkeypatch)
    srow, logw, prow, pidx, logq = got
    assert (logq < -10000).all() and np.isfinite(logw).all() and (np.diff(srow) == D.N_PATHS).all()
    assert (logw <= np.repeat(logq, D.N_PATHS) * (1.0 - 1e-12)).all()
    assert (np.diff(prow) >= 300).all()


def test_dense_sample_paths_never_choose_zero_mass(monkeypatch):
    """the most-used quarter of the parameters at -inf, an extra empty string,
    a string with an unemitted byte: no returned id has a -inf weight, strings
    own n paths or none exactly where the restatement says so"""
    fsa, w, sym, off, p = D.without_a_path_case()
    dev = _device(fsa, sym, off, p, monkeypatch)
    n = 16
    srow, logw, prow, pidx, logq = got = dev.dense_sample_paths(w, n, 9)
    want = D.sample_corpus(fsa, w, sym, off, n, 9)
    assert np.isfinite(w[pidx]).all()
    none = np.isneginf(want[4])
    assert none[-1] and none.any() and (~none).any()
    assert np.array_equal(np.isneginf(logq), none)
    assert np.array_equal(np.diff(srow), np.where(none, 0, n))
    assert np.isfinite(logw).all()
    _paths_equal(got, want, want[5], "without a path")
    _logq_close(logq, want[4])


def _qn_spec():
    return dict(n_states=16, degree=1, vocab=8, emissions=2, dense=True, n_strings=300, max_len=9, seed=21)


def test_dense_sampler_leaves_the_quasinewton_loop_alone(monkeypatch):
    """Run(3), Run(3) gives info rows bit-equal to Run(3), SamplePaths, Run(3)
    on a dense learner (rmin columns on); the learner's SamplePaths returns n
    paths per string"""
    import wfsa_amd as W
    monkeypatch.setenv("WFSA_DENSE", "1")
    syn = W.Synthetic(**_qn_spec())
    sym, off, wt = syn.corpus()
    fsa = W.Fsa.read_text(syn.wfsa_text)
    runs = []
    for sample in (False, True):
        lrn = W.QuasiNewtonLearner(0)
        lrn.set_info_rmin(True)
        lrn.BuildFromPacked(fsa, sym, off, wt)
        lrn.Finalize()
        lrn.Init(7)
        assert lrn.stats()["dense"] == 1
        rows = lrn.Run(3, 1.0, -1.0)
        if sample:
            srow, logw, prow, pidx, logq = lrn.SamplePaths(4, seed=11)
            assert (np.diff(srow) == 4).all() and len(srow) == len(wt) + 1
            assert np.isfinite(logw).all() and np.isfinite(logq).all() and (np.diff(prow) > 0).all()
            assert (logw <= np.repeat(logq, 4) + 1e-9).all()
        rows += lrn.Run(3, 1.0, -1.0)
        runs.append(np.array(rows))
    assert runs[0].shape == (6, 7)
    assert runs[0].tobytes() == runs[1].tobytes()
    assert W.HessianLearner.SamplePaths is W.QuasiNewtonLearner.SamplePaths


def test_dense_sampler_leaves_rmin_and_the_decode_result_alone(monkeypatch):
    import wfsa_amd as W
    from wfsa_amd import _lib
    fsa, w, sym, off, p = D.case("dense16")
    dev = _device(fsa, sym, off, p, monkeypatch)
    dev.recognize()
    rng = np.random.default_rng(9)
    w1 = rng.normal(-1.0, 0.5, size=dev.n_params)
    w2 = rng.normal(-1.0, 0.5, size=dev.n_params)
    dev.objective_grad(w1, want_logq=False)
    plain = dev.rmin()
    assert plain[1] >= 0
    dev.objective_grad(w1, want_logq=False)
    dev.dense_sample_paths(w2, 3, 1)
    assert dev.rmin() == plain
    # a dense_best_paths result fetched after a sampling call
    logw, prow, pidx = dev.dense_best_paths(w1)
    dev.dense_sample_paths(w2, 3, 2)
    prow2, pidx2 = np.zeros_like(prow), np.zeros(max(len(pidx), 1), dtype=np.int32)
    assert _lib.load().wfsa_dev_dense_best_paths_get(dev._h, prow2.ctypes.data, pidx2.ctypes.data) == 0
    assert prow2.tobytes() == prow.tobytes() and pidx2[:len(pidx)].tobytes() == pidx.tobytes()
    # and the decode after the sampler has used the shared history
    _same_bytes((logw, prow, pidx), dev.dense_best_paths(w1))
    ll, grad, logq = dev.objective_grad(w1)
    dev.dense_sample_paths(w2, 3, 3)
    ll2, grad2, logq2 = dev.objective_grad(w1)
    assert ll == ll2 and grad.tobytes() == grad2.tobytes() and logq.tobytes() == logq2.tobytes()


def test_cli_sample_paths_file_on_a_dense_model(tmp_path):
    """wfsa -sp 4 FILE on a dense model: as many rows and columns per string
    as the WFSA_DENSE=0 run, the strings in the same order"""
    import wfsa_amd as W
    syn = W.Synthetic(**dict(R.BYTE_CASES["dense16"][0], seed=21))
    sym, off, wt = syn.corpus()
    model, corpus = str(tmp_path / "dense16.wfsa"), str(tmp_path / "dense16.corpus")
    open(model, "wb").write(syn.wfsa_text.encode("latin-1"))
    with open(corpus, "wb") as f:
        f.write(b"\n")
        for i in range(len(wt)):
            f.write(bytes(sym[off[i]:off[i + 1]]) + b" %d\n" % int(wt[i]))
    rows = {}
    for dense in ("1", "0"):
        out = str(tmp_path / ("sample%s.tsv" % dense))
        r = subprocess.run([CLI, "-a", model, "-c", corpus, "-opt", "QuasiNewton", "-e", "3", "-i", "1", "-s", "-sp", "4", out,
                            "--sample-seed", "5"], capture_output=True, text=True, timeout=120, env=dict(os.environ, WFSA_DENSE=dense))
        assert r.returncode == 0, r.stderr[-2000:]
        lines = open(out, encoding="latin-1").read().split("\n")
        assert lines[-1] == ""
        rows[dense] = [l.split("\t") for l in lines[:-1]]
        assert len(rows[dense]) > 0 and all(len(row) == 5 for row in rows[dense])
    assert len(rows["1"]) == len(rows["0"]) and len(rows["1"]) % 4 == 0
    assert [row[:2] for row in rows["1"]] == [row[:2] for row in rows["0"]]
    for row in rows["1"]:
        assert len(row[4].split()) > 0 and float(row[3]) <= 1.0 + 1e-9


def test_dense_sample_paths_errors(monkeypatch):
    import wfsa_amd as W
    from wfsa_amd import _lib
    fsa, w0, sym, off, p = D.case("dense16")

    def arg_error(dev, w, word, n=2):
        with pytest.raises(W.WfsaError) as e:
            dev.dense_sample_paths(w, n, 0)
        assert e.value.code == _lib.WFSA_ERR_ARG and word in str(e.value), str(e.value)

    def get_rc(dev):
        srow = np.zeros(len(p) + 1, dtype=np.int64)
        return _lib.load().wfsa_dev_dense_sample_paths_get(dev._h, srow.ctypes.data, None, None, None)

    monkeypatch.setenv("WFSA_DENSE", "1")
    dev = W.Device(0)
    arg_error(dev, np.zeros(0), "load a model")              # nothing loaded
    dev.load_model(fsa)
    arg_error(dev, np.zeros(dev.n_params), "load a model")   # no corpus
    dev.load_corpus(sym, off, p)
    assert dev.stats()["dense"] == 1
    assert get_rc(dev) == _lib.WFSA_ERR_ARG                  # _get without a result since the load
    w = np.full(dev.n_params, -1.0)
    for n in (0, -1, 65):
        arg_error(dev, w, "n = %d" % n, n=n)
    for bad in (np.nan, np.inf):                             # a NaN or +inf weight (-inf is allowed)
        wb = w.copy()
        wb[dev.n_params // 2] = bad
        arg_error(dev, wb, "NaN or +inf")
    dev.recognize()
    dev.objective_grad_begin(w)                              # while an evaluation is in flight
    arg_error(dev, w, "in flight")
    dev.objective_grad_end()
    srow, logw, prow, pidx, logq = dev.dense_sample_paths(w, 2, 0)
    assert np.isfinite(logw).all() and get_rc(dev) == 0
    dev.load_corpus(sym, off, p)                             # a load ends the result
    assert get_rc(dev) == _lib.WFSA_ERR_ARG
    with pytest.raises(W.WfsaError) as e:                    # the trellis entry point keeps its contract
        dev.sample_paths(w, 2, 0)
    assert e.value.code == _lib.WFSA_ERR_CAPACITY and "WFSA_DENSE=0" in str(e.value)
    dev.load_paths(2, [0, 1, 2], [0, 1], [1.0, 1.0], [0, 2], [0, 1], [1.0])   # matrix-file mode: no automaton
    arg_error(dev, np.zeros(2), "matrix")
    sp = _device(fsa, sym, off, p, monkeypatch, dense=False)  # not on the dense path: the other entry point serves it
    arg_error(sp, w, "wfsa_dev_sample_paths")
    assert np.isfinite(sp.sample_paths(w, 2, 0)[1]).all()


def test_dense_sample_paths_stats(monkeypatch):
    fsa, w, sym, off, p = D.case("dense16")
    dev = _device(fsa, sym, off, p, monkeypatch)
    dev.dense_sample_paths(w, 4, 0)
    st = dev.stats()
    assert st["sample_path_ms"] > 0.0 and st["dense_sp_forward_ms"] > 0.0 and st["dense_sp_backward_ms"] > 0.0
    parts = st["dense_sp_forward_ms"] + st["dense_sp_backward_ms"]
    assert abs(parts - st["sample_path_ms"]) <= 1e-9 * st["sample_path_ms"]
