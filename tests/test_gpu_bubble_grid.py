"""The bubble-grid form of the stream-less step launch (fb_kernels.hip
step_grid_kernel) against step_dot_kernel's geometry, bit for bit.

The grid launches only the waves that have work, longest first, and leaves
the block partials to the kernel that follows (the reduction, qn_wave_kernel
or qn_step_kernel); nothing in a wave's arithmetic changes, so with
WFSA_BUBBLE_GRID=1 (the default) and =0 the info rows, x, last_grad and
objective_grad()'s KL and gradient must have the same bytes.  The knob is read
when a context is created: each setting runs in a fresh context, as the other
knob tests do.

The corpora: the `ambiguous` family (mixed-structure class-B waves, id-0
bubbles) and a family-A corpus of 20,000 strings (a partial last class-A
wave, few class-B waves), both test_gpu_ll_dot.py's shapes, with its
sparse-use shape (a parameter Trim dropped: weight -inf, coefficient 0); and
corpora built by hand from bubble_gadgets.py's gadgets, whose class counts
stats() must report as stated here.
"""
import numpy as np
import pytest

import bubble_gadgets as B
import test_gpu_ll_dot as L

pytestmark = pytest.mark.gpu

KNOBS = ("WFSA_BUBBLE_GRID", "WFSA_QN_INKERNEL", "WFSA_QN_WAVE", "WFSA_LL_DOT", "WFSA_BUBBLE_SHAPES", "WFSA_GRAPH")


@pytest.fixture(scope="module", autouse=True)
def _release_corpora():
    yield
    L._corpora.clear()   # (the model handles go before the interpreter shuts down)
    _hand.clear()


def _prefix(i):
    """eight unary visits that spell i: distinct strings around the same bubbles"""
    return [("u1", "v1")[i >> b & 1] for b in range(8)]


# name -> (specs, the class counts stats() must report: A, B, big)
def _hand_specs(name):
    if name == "class_a":      # 70 diamonds mid-string, 3 at the string's end: two chunks, the last partial
        return [(_prefix(i) + ["d2"], False) for i in range(70)] + [(_prefix(i) + ["d2"], True) for i in range(3)], (73, 0, 0)
    if name == "class_b":      # five structures (one without compiled sweeps) through two chunks: mixed-structure waves
        gs = ["t3", "c22", "q4", "c222", "f22"]
        return [(_prefix(i) + [gs[i % 5]], bool(i & 1)) for i in range(75)], (0, 75, 0)
    if name == "big":          # fewer big bubbles than any launch has waves
        return [(_prefix(i) + [g], False) for i, g in enumerate(["c33", "s6", "c2222", "s7", "s6"])], (0, 0, 5)
    if name == "one":          # one bubble in all, among strings without any
        return [(["t3"], False)] + [(_prefix(i), False) for i in range(1, 6)], (0, 1, 0)
    if name == "none":         # no bubble at all: the launch is the dot product alone
        return [(_prefix(i), False) for i in range(1, 9)], (0, 0, 0)
    if name == "big_many":     # 256 big bubbles in 128 strings: more than the waves of the geometry (the
                               # test asserts it from stats()), so a big-bubble role loops
        return [(_prefix(i) + ["s6", "c33"], bool(i & 1)) for i in range(128)], (0, 0, 256)
    raise KeyError(name)


HAND = ["class_a", "class_b", "big", "one", "none", "big_many"]
_hand = {}


def _hand_case(W, name):
    if name not in _hand:
        specs, counts = _hand_specs(name)
        c = B.Case(specs)
        _hand[name] = (W.Fsa.read_text(c.text), c.sym, c.off, c.wt, counts)
    return _hand[name]


def _learner(W, corpus, monkeypatch, grid, rmin=False, env=None):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if grid is not None:
        monkeypatch.setenv("WFSA_BUBBLE_GRID", grid)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    lrn = W.QuasiNewtonLearner(0)
    lrn.set_info_rmin(rmin)
    lrn.BuildFromPacked(*corpus)
    lrn.Finalize()
    lrn.Init(7)
    return lrn


def _trace(lrn, steps, seed=None):
    """the step path and the evaluation path from one start: the rows of
    Run(steps), x, last_grad, then objective_grad()'s KL and gradient; the
    launches counted across them"""
    if seed is not None:   # off the initial point, the same move under both settings
        lrn.set_x(lrn.x() + np.random.default_rng(seed).normal(0.0, 0.5, size=len(lrn.x())))
    s0 = lrn.stats()
    rows = np.array(lrn.Run(steps, 1.0, -1.0), dtype=np.float64)
    x, grad = lrn.x(), lrn.last_grad()
    kl, g, _ = lrn.objective_grad()
    s1 = lrn.stats()
    counts = {k: s1[k] - s0[k] for k in ("ll_dot_launches", "bubble_grid_launches", "qn_wave_launches")}
    return dict(rows=rows, x=x, grad=grad, kl=np.array([kl], dtype=np.float64), g=np.asarray(g, dtype=np.float64)), counts, s1


def _assert_same_bytes(a, b, tag):
    for k in ("rows", "x", "grad", "kl", "g"):
        u, v = a[k], b[k]
        assert u.shape == v.shape, (tag, k, u.shape, v.shape)
        bad = np.flatnonzero(u.view(np.uint64).ravel() != v.view(np.uint64).ravel())
        assert bad.size == 0, f"{tag}: {k} differs at {bad[:8].tolist()}: {u.ravel()[bad[:4]]} vs {v.ravel()[bad[:4]]}"
        assert u.tobytes() == v.tobytes(), (tag, k)


def _compare(W, corpus, monkeypatch, steps, tag, seed=None, env=None):
    new, n_new, st = _trace(_learner(W, corpus, monkeypatch, "1", env=env), steps, seed)
    old, n_old, _ = _trace(_learner(W, corpus, monkeypatch, "0", env=env), steps, seed)
    print(f"{tag}: launches grid {n_new} geometry {n_old}; KL {new['kl'][0]!r}; bubbles A {st['small_bubbles_a']} "
          f"B {st['small_bubbles_b']} big {st['big_bubbles']} mixed waves {st['mixed_shape_waves']} "
          f"fused {st['bubbles_fused']} block {st['stream_block']}")
    assert np.isfinite(new["kl"]).all() and np.isfinite(new["rows"][:, :5]).all()
    # every stream-less launch of the run took the grid form (steps + the evaluation), none with the knob off
    assert n_new["bubble_grid_launches"] == n_new["ll_dot_launches"] == steps + 1, n_new
    assert n_old["bubble_grid_launches"] == 0 and n_old["ll_dot_launches"] == steps + 1, n_old
    _assert_same_bytes(new, old, tag)
    return new, st


@pytest.mark.parametrize("qn_wave", ["1", "0"], ids=["qn_wave", "qn_step"])
@pytest.mark.parametrize("shape", ["ambiguous", "A-small", "sparse-use"])
def test_synthetic_families_keep_their_bits(shape, qn_wave, monkeypatch):
    """five QN steps and one objective_grad(); the block partials summed by
    qn_wave_kernel, by qn_step_kernel (WFSA_QN_WAVE=0) and by the reduction"""
    import wfsa_amd as W
    corpus = L._corpus(W, shape)[1:]
    new, st = _compare(W, corpus, monkeypatch, 5, f"{shape} WFSA_QN_WAVE={qn_wave}",
                       env={"WFSA_QN_WAVE": qn_wave, "WFSA_QN_INKERNEL": "0"})
    if shape == "ambiguous":
        assert st["mixed_shape_waves"] > 0 and st["shaped_bubbles"] < st["small_bubbles_a"] + st["small_bubbles_b"]
    if shape == "A-small":
        assert st["small_bubbles_a"] % 64 != 0 and 0 < st["small_bubbles_b"] < st["small_bubbles_a"]
    if shape == "sparse-use":   # else the shape proves nothing about the -inf guard
        lrn = _learner(W, corpus, monkeypatch, "1")
        assert (lrn.trimmed_index() == -2).any(), "no parameter was trimmed as unused"


@pytest.mark.parametrize("name", HAND)
def test_hand_built_corpora_keep_their_bits(name, monkeypatch):
    """one class at a time, one bubble, none, and more big bubbles than
    waves, at three weight draws: three QN steps and one objective_grad()"""
    import wfsa_amd as W
    fsa, sym, off, wt, (na, nb, nbig) = _hand_case(W, name)
    for seed in B.SEEDS:
        _, st = _compare(W, (fsa, sym, off, wt), monkeypatch, 3, f"{name} seed {seed}", seed=seed)
        assert (st["small_bubbles_a"], st["small_bubbles_b"], st["big_bubbles"]) == (na, nb, nbig)
        assert st["fallback_strings"] == 0
        if name == "class_b":
            assert st["mixed_shape_waves"] > 0
        # the geometry's waves (a role is one of them); a big-bubble rank takes bubbles rank, rank + waves - 1, ...
        waves = st["stream_grid"] * (st["stream_block"] // 64)
        assert waves >= 2 and st["bubbles_fused"] == (1 if na + nb + nbig else 0)
        if name == "big":
            assert nbig < waves - 1, (nbig, waves)    # no rank takes a second bubble
        if name == "big_many":
            assert nbig > waves - 1, (nbig, waves)    # some rank's loop takes a second bubble


def test_default_is_the_grid(monkeypatch):
    import wfsa_amd as W
    corpus = L._corpus(W, "A-small")[1:]
    _, n, _ = _trace(_learner(W, corpus, monkeypatch, None), 2)
    assert n["bubble_grid_launches"] == n["ll_dot_launches"] == 3, n


def test_a_halted_launch_stores_nothing(monkeypatch):
    """as test_gpu_step_entry's: the launches enqueued behind a halt return at
    once -- the grid's roles and the kernels that sum its partials store
    nothing that shows, and the halted run equals the geometry's"""
    import wfsa_amd as W
    corpus = L._corpus(W, "A-small")[1:]
    free = np.array(_learner(W, corpus, monkeypatch, "1").Run(10, 1.0, -1.0))
    gerr = free[:, 1]
    assert gerr[2] < gerr[1], gerr
    tol = 0.5 * (gerr[1] + gerr[2])   # between rows 2 and 3
    within = (free[:, 1] <= tol) & (np.abs(free[:, 2]) <= tol) & (np.abs(free[:, 3]) <= tol)
    assert not within[:2].any() and within[2:6].any(), free[:, 1:4]
    h = int(np.flatnonzero(within)[0]) + 1
    out = {}
    for tag, grid, steps, t in (("halted", "1", 10, tol), ("exact", "1", h, -1.0), ("geometry", "0", 10, tol)):
        lrn = _learner(W, corpus, monkeypatch, grid)
        rows = np.array(lrn.Run(steps, 1.0, t), dtype=np.float64)
        kl, g, _ = lrn.objective_grad()
        out[tag] = dict(rows=rows, x=lrn.x(), grad=lrn.last_grad(), kl=np.array([kl]), g=np.asarray(g))
        assert (lrn.stats()["bubble_grid_launches"] > 0) == (grid == "1")
    assert len(out["halted"]["rows"]) == h, f"halted after {len(out['halted']['rows'])} steps, not {h}"
    assert out["halted"]["rows"].tobytes() == free[:h].tobytes()
    _assert_same_bytes(out["halted"], out["exact"], "halted vs ran exactly to the halt")
    _assert_same_bytes(out["halted"], out["geometry"], "halted vs WFSA_BUBBLE_GRID=0")


def test_other_variants_keep_the_geometry(monkeypatch):
    """the rmin column and the in-kernel QN update need step_dot_kernel's
    hand-offs: their steps never take the grid.  (The counter is compared
    across Run: preparing a learner evaluates the objective once, without the
    column and outside any step -- step_dot_kernel<false, false, false>'s
    work, which the grid takes.)"""
    import wfsa_amd as W
    corpus = L._corpus(W, "A-small")[1:]
    lrn = _learner(W, corpus, monkeypatch, "1", rmin=True, env={"WFSA_QN_INKERNEL": "0"})
    s0 = lrn.stats()
    lrn.Run(3, 1.0, -1.0)
    s1 = lrn.stats()
    assert s1["ll_dot_launches"] - s0["ll_dot_launches"] == 3
    assert s1["bubble_grid_launches"] - s0["bubble_grid_launches"] == 0, (s0["bubble_grid_launches"], s1["bubble_grid_launches"])
    lrn = _learner(W, corpus, monkeypatch, "1", env={"WFSA_QN_INKERNEL": "1"})
    s0 = lrn.stats()
    lrn.Run(3, 1.0, -1.0)
    s1 = lrn.stats()
    assert s1["qn_inkernel_waves"] > 0, "the in-kernel update did not run"
    assert s1["ll_dot_launches"] - s0["ll_dot_launches"] == 3
    assert s1["bubble_grid_launches"] - s0["bubble_grid_launches"] == 0, (s0["bubble_grid_launches"], s1["bubble_grid_launches"])
