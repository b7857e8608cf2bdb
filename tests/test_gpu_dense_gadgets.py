"""The dense path (dense_path.hip, dense_decode.hip) on automata built by hand
(dense_gadgets.py): holes in A, in the start row and in the end column,
single-member groups, ^ -> $ with the empty string, strings that die, states
at the column-tile edges, three column tiles, two to four row tiles chosen on
purpose, T = 1 and T = 2, runs of length-1 strings in one slot, vocabularies
of two and three reduce windows, log q near -12000 and posteriors of 4e-18.

Every gadget runs on the four GEMM engines.  stats() confirms the row slots,
steps and padded width the gadget was built for.  Recognition, path counts,
used parameters, log q, the log-likelihood, the gradient and rmin are held to
dense_gadgets.reference (long double, per string) at test_gpu_dense's bounds
-- log q and LL rel 1e-12, gradient rtol 1e-10 atol 1e-17, rmin rel 1e-11; for
long300, peaked and tiles384 the larger of those and 16 times the distance of
a float64 numpy restatement from the reference, measured where the test runs
(profiles/dense_gadgets/errors.json).  A parameter the reference gives 0 must
be exactly 0.0.  test_dense_gadgets_reference.py holds the reference to the
oracle and shows what the gadgets can tell apart.  Each test prints its worst
relative errors.  Needs a gfx950 device."""
import numpy as np
import pytest

import dense_gadgets as G

pytestmark = pytest.mark.gpu

BITWISE = ("holes12", "edge129", "seams", "vocab65")


@pytest.fixture(autouse=True, params=["fused", "split", "dma", "blas"])
def gemm_engine(request, monkeypatch):
    """every test on the four GEMM engines of the dense path (test_gpu_dense.py)"""
    monkeypatch.delenv("WFSA_DENSE_BLAS", raising=False)
    monkeypatch.setenv("WFSA_DENSE_ENGINE", request.param)
    monkeypatch.setenv("WFSA_DENSE", "1")
    return request.param


def _memo(fn):
    cache = {}

    def wrapped(*key):
        if key not in cache:
            cache[key] = fn(*key)
        return cache[key]
    wrapped.cache_clear = cache.clear
    return wrapped


def _subset(g, keep):
    strings = [bytes(g.sym[g.off[i]:g.off[i + 1]]) for i in keep]
    sym = np.frombuffer(b"".join(strings), dtype=np.uint8).copy()
    off = np.concatenate([[0], np.cumsum([len(s) for s in strings])]).astype(np.int64)
    return sym, off, g.p[keep]


@_memo
def _case(name):
    """(gadget, fsa, weights, reference of the whole corpus, the recognized
    strings (sym, off, p), their reference, the bounds), computed once and left unchanged"""
    import wfsa_amd as W
    g = G.GADGETS[name]()
    fsa = W.Fsa.read_text(g.text.encode("latin-1"))
    w = G.weights(g, fsa.param_names())
    whole = G.reference(fsa, w, g.sym, g.off, g.p)
    keep = np.flatnonzero([k > 0 for k in whole.paths])
    sub = _subset(g, keep)
    ref = G.reference(fsa, w, *sub) if len(keep) < len(g.p) else whole
    f64 = (0.0, 0.0, 0.0)
    if name in G.LOOSENED:
        logq, _, grad, rmin = G.restate(fsa, w, *sub)
        some = np.diff(sub[1]) > 0
        f64 = (G.distance(logq, ref.logq), G.distance(grad, ref.grad, G.GRAD_ATOL), G.distance(rmin[some], ref.rmin[some]))
        print(f"dense_gadgets f64 distance | {name} | logq {f64[0]:.3e} grad {f64[1]:.3e} rmin {f64[2]:.3e}")
    for r in (whole, ref):
        for a in (r.logq, r.grad, r.rmin, r.used):
            a.setflags(write=False)
    return g, fsa, w, whole, keep, sub, ref, G.bounds(name, f64)


@pytest.fixture(scope="module", autouse=True)
def _drop_caches():
    yield
    _case.cache_clear()
    for f in G.GADGETS.values():
        if hasattr(f, "cache_clear"):
            f.cache_clear()


ERRORS = {}


def _note(name, engine, **errs):
    worst = ERRORS.setdefault((name, engine), {})
    for k, v in errs.items():
        worst[k] = max(worst.get(k, 0.0), v)
    print(f"dense_gadgets worst rel err | {name} | {engine} | " + " ".join(f"{k} {v:.3e}" for k, v in sorted(worst.items())))


def _device(fsa, sym, off, p, shape=None, npad=None):
    import wfsa_amd as W
    dev = W.Device(0)
    dev.load_model(fsa)
    dev.load_corpus(sym, off, p)
    st = dev.stats()
    assert st["dense"] == 1
    if shape is not None:
        assert (st["dense_rows"], st["dense_steps"], st["dense_np"]) == (*shape, npad), st
    return dev


def _check_weighted(name, engine, dev, w, ref, off, lim, tag=""):
    """objective_grad and rmin against the reference of the loaded strings"""
    lq_rel, g_rel, r_rel = lim
    ll, grad, logq = dev.objective_grad(w)
    some = np.diff(off) > 0
    live = np.isfinite(ref.logq) & some
    errs = {tag + "logq": G.distance(logq, ref.logq), tag + "ll": G.distance(ll, ref.ll),
            tag + "grad": G.distance(grad, ref.grad, G.GRAD_ATOL)}
    r, s = dev.rmin()
    if live.any():
        want = np.where(live, ref.rmin, np.inf)
        i = int(np.argmin(want))
        errs[tag + "rmin"] = G.distance(r, want[i])
    _note(name, engine, **errs)
    assert G.close(logq, ref.logq, lq_rel)
    assert G.close(ll, ref.ll, lq_rel)
    assert G.close(grad, ref.grad, g_rel, G.GRAD_ATOL)
    zero = ref.grad == 0
    assert (grad[zero] == 0.0).all()
    assert np.array_equal(zero, ~ref.used)
    if live.any():
        assert G.close(r, want[i], r_rel)
        assert s == i or (live[s] and G.close(want[s], want[i], r_rel))
    else:
        assert s == -1
    return ll, grad, logq


@pytest.mark.parametrize("name", G.GADGETS)
def test_gadget(name, gemm_engine):
    g, fsa, w, whole, keep, sub, ref, lim = _case(name)
    dev = _device(fsa, g.sym, g.off, g.p, (g.R, g.T), g.notes["np"])
    rec, pc, used = dev.recognize()
    paths = np.array([float(k) for k in whole.paths])
    assert np.array_equal(rec.astype(bool), paths > 0)
    assert G.close(pc, paths, 1e-12) and (pc[paths == 0] == 0.0).all()
    assert np.array_equal(used.astype(bool), whole.used)
    # the recognized strings, reloaded as the Learner does (the empty string kept)
    sym, off, p = sub
    if len(keep) < len(g.p):
        assert name == "holes12" and (np.diff(off) == 0).sum() == 1
        R, T, _ = G.slot_shape(np.diff(off), g.notes["np"])
        dev = _device(fsa, sym, off, p, (R, T), g.notes["np"])
    ll, grad, logq = _check_weighted(name, gemm_engine, dev, w, ref, off, lim)
    if name == "t1":   # no GEMM ran: no interior transition has a count
        from dense_decode_reference import Tables
        pA = Tables(fsa, w).pA
        assert (grad[pA[pA >= 0]] == 0.0).all()
    if name in BITWISE:
        from dense_decode_reference import decode_corpus
        ll2, grad2, logq2 = dev.objective_grad(w)
        assert ll2 == ll and np.array_equal(grad2, grad) and np.array_equal(logq2, logq)
        logw, prow, pidx = dev.dense_best_paths(w)
        want, wrow, widx, _, _ = decode_corpus(fsa, w, sym, off)
        assert np.array_equal(logw, want)
        assert len(prow) == len(wrow) and prow[-1] == len(pidx)


def test_holes12_dead_strings_left_in(gemm_engine):
    """the whole corpus loaded, p = 0 on the strings no path accepts: their
    log q is -inf, they add nothing to LL and the gradient, and the string
    that follows one in its slot is not disturbed"""
    g, fsa, w, whole, keep, sub, ref, lim = _case("holes12")
    p = g.p.copy()
    p[g.notes["dead"]] = 0.0
    dev = _device(fsa, g.sym, g.off, p, (g.R, g.T), g.notes["np"])
    rec, _, _ = dev.recognize()
    assert not rec[g.notes["dead"]].any() and rec.sum() == len(keep)
    want = G.reference(fsa, w, g.sym, g.off, p)
    assert (want.logq[g.notes["dead"]] == -np.inf).all() and np.isfinite(want.ll)
    ll, grad, logq = _check_weighted("holes12", gemm_engine, dev, w, want, g.off, lim, tag="dead_")
    assert (logq[g.notes["dead"]] == -np.inf).all()
    # the same with p > 0 on them: LL is -inf, the gradient unchanged
    dev.load_corpus(g.sym, g.off, g.p)
    ll, grad, logq = dev.objective_grad(w)
    assert ll == -np.inf and G.close(logq, whole.logq, lim[0]) and G.close(grad, whole.grad, lim[1], G.GRAD_ATOL)


def test_automatic_choice(gemm_engine, monkeypatch):
    """dense_model_build's admission rule at its edge: 64 interior states and
    4 n_tr >= n^2; forced, a model it cannot hold stays on the trellis kernels"""
    import wfsa_amd as W

    def dense(text):
        dev = W.Device(0)
        dev.load_model(W.Fsa.read_text(text))
        return dev.stats()["dense"]
    monkeypatch.delenv("WFSA_DENSE", raising=False)
    assert dense(G.choice_model(64, 16)) == 1
    assert dense(G.choice_model(64, 16, drop=1)) == 0
    assert dense(G.choice_model(63, 63)) == 0
    monkeypatch.setenv("WFSA_DENSE", "1")
    assert dense(G.choice_model(63, 63)) == 1
    assert dense(G.two_byte_model()) == 0
    assert dense(G.epsilon_model()) == 0
