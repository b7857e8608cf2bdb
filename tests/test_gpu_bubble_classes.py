"""The bubble kernels on bubbles chosen by hand (bubble_gadgets.py): the class
boundaries, the compile limits, the big bubbles' branches and the lane groups.

The other bubble tests draw their automata from Synthetic(...), so which
bubbles they meet is an accident of a seed, and most of them compare the
kernels with themselves.  Here every corpus is built from gadgets whose
bubbles have stated sizes: the counts stats() reports are computed from the
strings' visits without the device, and every evaluation path is held to the
ENUM oracle at the same weights (Init(7) plus the perturbation of
test_gpu_regimes, three draws), at the tolerances of
test_gpu_regimes._check_evaluation and
test_device_qn_loop_matches_oracle_steps.  test_bubble_gadgets_reference.py
shows that the oracle itself is inside those tolerances of a long-double sum
over the enumerated paths.
"""
import numpy as np
import pytest

import bubble_gadgets as B

pytestmark = pytest.mark.gpu

COUNTERS = ("small_bubbles_a", "small_bubbles_b", "big_bubbles", "shaped_bubbles", "fallback_strings",
            "max_bubble_nodes", "max_bubble_edges")
REGIME_KEYS = ("stream_block", "stream_w_lds", "stream_wide", "stream_multi", "stream_delta", "bubbles_fused")
KNOBS = ("WFSA_LL_DOT", "WFSA_BUBBLE_SHAPES", "WFSA_SLOT_MERGE", "WFSA_QN_INKERNEL")
# the evaluation settings: environment, rmin column
SETTINGS = {
    "default": ({}, False),
    "ll_dot_off": ({"WFSA_LL_DOT": "0"}, False),   # the stream kernel holds the bubbles, fused or not
    "shapes_off": ({"WFSA_BUBBLE_SHAPES": "0"}, False),
    "rmin": ({}, True),
}

# the limit corpus' regimes (bubble_gadgets.LIMITS_PAD): 16 waves' staging of 3,584 bytes fits beside
# a table of 8 bytes per parameter in 162,816 bytes up to about 13,180 parameters
LIMIT_REGIMES = {
    "limits": dict(stream_block=512, stream_w_lds=1, bubbles_fused=1),
    "limits_12k": dict(stream_block=1024, stream_w_lds=1, bubbles_fused=1),
    "limits_14k": dict(stream_block=1024, stream_w_lds=1, bubbles_fused=0),
    "limits_23k": dict(stream_w_lds=0, bubbles_fused=0),
}


@pytest.fixture(scope="module", autouse=True)
def _drop_caches():
    """the corpora and references are shared by this module's tests only"""
    yield
    for cached in (B.reference, B.case, B.lanes, _fsa):
        cached.cache_clear()


def _close(a, b, rel, atol=1e-13):
    return abs(a - b) <= max(atol, rel * max(abs(a), abs(b)))


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = np.maximum(np.abs(a), np.abs(b))
    return float(np.max(np.where(d > 0, np.abs(a - b) / np.where(d > 0, d, 1.0), 0.0))) if a.size else 0.0


def _regime(st):
    return {k: st[k] for k in REGIME_KEYS}


def _memo(fn):
    cache = {}

    def wrapped(key):
        if key not in cache:
            cache[key] = fn(key)
        return cache[key]
    wrapped.cache_clear = cache.clear
    return wrapped


@_memo
def _fsa(key):
    import wfsa_amd as W
    return W.Fsa.read_text(B.get(key).text)


def _learner(key, monkeypatch, env=None, rmin=False):
    import wfsa_amd as W
    c = B.get(key)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    lrn = W.QuasiNewtonLearner(0)
    lrn.set_info_rmin(rmin)
    lrn.BuildFromPacked(_fsa(key), c.sym, c.off, c.wt)
    lrn.Finalize()
    lrn.Init(7)
    return lrn


def _perturb(lrn, key, seed):
    """Init(7) plus the draw's step, by name; returns the learner's names"""
    step = B.reference(key, seed)[0]
    dn = lrn.param_names()
    assert sorted(dn) == sorted(step)
    lrn.Init(7)
    lrn.set_x(lrn.x() + np.array([step[n] for n in dn]))
    return dn


def _check_evaluation(key, lrn, seed, tag=""):
    """KL and the gradient from objective_grad(), and KL, the gradient and
    log q of every string from objective_grad(want_logq=True), against ENUM
    at the draw's weights"""
    _, kl_o, g_o, logq_o = B.reference(key, seed)
    dn = _perturb(lrn, key, seed)
    kl, g, _ = lrn.objective_grad()
    kl2, g2, logq = lrn.objective_grad(want_logq=True)
    by, by2 = dict(zip(dn, g)), dict(zip(dn, g2))
    keys = sorted(by)   # (reference()'s order)
    g_d, g2_d = np.array([by[k] for k in keys]), np.array([by2[k] for k in keys])
    print(f"{key} {tag} seed {seed}: rel err vs ENUM: KL {abs(kl - kl_o) / abs(kl_o):.2e} grad {_rel(g_d, g_o):.2e} "
          f"(abs {np.abs(g_d - g_o).max():.2e}) logq {_rel(logq, logq_o):.2e}; with logq: KL "
          f"{abs(kl2 - kl_o) / abs(kl_o):.2e} grad {_rel(g2_d, g_o):.2e}")
    assert np.isfinite(logq_o).all() and np.isfinite(g_o).all()
    assert _close(kl, kl_o, rel=1e-11)
    np.testing.assert_allclose(g_d, g_o, rtol=1e-10, atol=1e-15)
    assert logq.shape == logq_o.shape
    np.testing.assert_allclose(logq, logq_o, rtol=1e-12, atol=1e-12)
    assert _close(kl2, kl_o, rel=1e-11)
    np.testing.assert_allclose(g2_d, g_o, rtol=1e-10, atol=1e-15)


def _check_rmin_row(key, lrn, o, on, dn):
    """one device step at the learner's own x: its KL column, the rmin column
    (1e-12 relative) and the string the column names, against the oracle's
    path matrices at exactly those weights"""
    x = dict(zip(dn, lrn.x()))
    row = lrn.Run(1, 1.0, -1.0)[0]
    want, rpp, mrow = B.oracle_rmin(o, np.array([x[n] for n in on]))
    s = int(row[6])
    print(f"{key}: rmin {row[5]:.17g} want {want:.17g} rel err {abs(row[5] - want) / want:.2e} string {s}")
    assert abs(row[5] - want) <= 1e-12 * want, (row[5], want)
    assert 0 <= s < len(mrow) - 1 and mrow[s + 1] - mrow[s] > 1   # an ambiguous string holding that minimum
    assert abs(rpp[mrow[s]:mrow[s + 1]].min() - want) <= 1e-12 * want
    return row, s


# -- classification ------------------------------------------------------------

def _device_counts(key, monkeypatch, env):
    import wfsa_amd as W
    c = B.get(key)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    fsa = _fsa(key)
    dev = W.Device(0)
    dev.load_model(fsa)
    dev.load_corpus(c.sym, c.off, c.wt / c.wt.sum())
    rec, pc, _ = dev.recognize()
    assert rec.all() and np.array_equal(pc, c.path_counts())
    dev.objective_grad(np.full(len(fsa.param_names()), -1.0), want_logq=False)
    return dev.stats(), dev.string_tiers()


@pytest.mark.parametrize("key", ["all", "big", "big1", "limits", "limits_14k", "mixed", "mixed_m2", 65])
def test_classification_is_exact(key, monkeypatch):
    """the class counts, the bubbles with a compiled-in structure, the
    traversal strings and the largest bubble equal the numbers computed from
    the strings' visits; WFSA_BUBBLE_SHAPES=0 changes the structure ids alone"""
    c = B.get(key)
    want = c.expected()
    st, tiers = _device_counts(key, monkeypatch, {})
    st0, tiers0 = _device_counts(key, monkeypatch, {"WFSA_BUBBLE_SHAPES": "0"})
    got, got0 = {k: st[k] for k in COUNTERS}, {k: st0[k] for k in COUNTERS}
    print(f"{key}: expected {want}")
    print(f"{key}: default  {got} n_bubbles {st['n_bubbles']} compiled {st['compiled_strings']} "
          f"bubbles_fused {st['bubbles_fused']} regime {_regime(st)}")
    print(f"{key}: WFSA_BUBBLE_SHAPES=0 {got0} bubbles_fused {st0['bubbles_fused']}")
    assert got == want
    assert got0 == dict(want, shaped_bubbles=0)
    assert st["n_bubbles"] == want["small_bubbles_a"] + want["small_bubbles_b"] + want["big_bubbles"]
    assert st["compiled_strings"] == len(c.strings) - want["fallback_strings"]
    # the strings past the compile limits, and only they, run on a traversal tier
    assert np.array_equal(tiers >= 0, c.traversal()) and np.array_equal(tiers0, tiers)
    if key == "all":
        assert got["max_bubble_nodes"] == 32 and got["max_bubble_edges"] == 255 and got["fallback_strings"] == 3


# -- every evaluation path against the oracle -------------------------------------

@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("key", ["all", "big", "big1", "limits"] + list(B.LIMITS_PAD))
def test_evaluation_matches_enum(key, setting, monkeypatch):
    """objective_grad() and objective_grad(want_logq=True) at three weight
    draws: by default (the stream-less launch holds the bubbles), with
    WFSA_LL_DOT=0 (the stream kernel does), on the generic sweeps alone, and
    with the rmin column on -- there also one device step's rmin column at
    the draw's weights.  all and big hold the two-emission diamond (a model
    with a multi-parameter edge keeps the 16-bit streams), big1 and limits do
    not (the delta format).  The limit corpus must pass whichever way
    bubbles_fused falls: its staging is big_stage_bytes(256) per wave, and
    with the automaton's parameter count raised by states no string reaches
    (LIMIT_REGIMES) it fits beside the staged weights in a 1024-thread block,
    does not fit, or the weights are not staged at all"""
    env, rmin = SETTINGS[setting]
    lrn = _learner(key, monkeypatch, env, rmin)
    want = B.get(key).expected()
    for seed in B.SEEDS:
        _check_evaluation(key, lrn, seed, setting)
    st = lrn.stats()
    print(f"{key} {setting}: bubbles_fused {st['bubbles_fused']} ll_dot_launches {st['ll_dot_launches']} "
          f"regime {_regime(st)} big {st['big_bubbles']} max edges {st['max_bubble_edges']}")
    if setting == "shapes_off":
        want = dict(want, shaped_bubbles=0)
    assert {k: st[k] for k in COUNTERS} == want
    if not any(B.GADGETS[n].multi for n in B.get(key).names):
        assert st["stream_multi"] == 0 and st["stream_delta"] == st["stream_w_lds"]
    if key in LIMIT_REGIMES:
        assert {k: st[k] for k in LIMIT_REGIMES[key]} == LIMIT_REGIMES[key], _regime(st)
    # both WFSA_LL_DOT settings ran: the evaluations without log q took the stream-less launch, or none did
    if setting == "ll_dot_off":
        assert st["ll_dot_launches"] == 0
    else:
        assert st["ll_dot_launches"] >= len(B.SEEDS), "the stream-less launch did not run"
    if rmin:
        o, on, _ = B.perturbed_oracle(key, B.SEEDS[0])
        dn = _perturb(lrn, key, B.SEEDS[0])
        row, _ = _check_rmin_row(key, lrn, o, on, dn)
        assert _close(row[0], B.reference(key, B.SEEDS[0])[1], rel=1e-11)


# -- device-resident steps -----------------------------------------------------

@pytest.mark.parametrize("rmin", [False, True], ids=["", "rmin"])
@pytest.mark.parametrize("inkernel", [0, 1], ids=["two_kernels", "one_launch"])
@pytest.mark.parametrize("key", ["mixed", "mixed_m2"])
def test_device_steps_match_oracle_steps(key, inkernel, rmin, monkeypatch):
    """Run(3, 1.0, -1.0) against three qn_step(1.0) of the oracle from each
    weight draw, on strings of one, two and three bubbles of mixed classes
    (the per-string sums of log Z and of the rmin column run over class-A and
    class-B lanes and big-bubble waves); with the rmin column on, the column
    and its string at the device's own x, one step more.  mixed runs on the
    delta format, where WFSA_QN_INKERNEL=1 puts the QN update into the step's
    one launch; mixed_m2 holds the two-emission diamond and keeps the 16-bit
    streams and the separate QN kernel"""
    c = B.get(key)
    lrn = _learner(key, monkeypatch, {"WFSA_QN_INKERNEL": str(inkernel)}, rmin)
    n_bub = np.array([len(bs) for bs in c.bubbles()])
    assert len(n_bub) == len(c.strings) and set(n_bub) == {1, 2, 3}
    min_on_multi = []
    for seed in B.SEEDS:
        o, on, _ = B.perturbed_oracle(key, seed)
        dn = _perturb(lrn, key, seed)
        assert sorted(dn) == sorted(on)
        want_rmin, orows = [], []
        for _ in range(3):
            want_rmin.append(B.oracle_rmin(o, o.x())[0])
            orows.append(o.qn_step(1.0))
        rows = lrn.Run(3, 1.0, -1.0)
        assert len(rows) == 3
        st = lrn.stats()
        da, oa = np.array(rows)[:, :5], np.array(orows)[:, :5]
        print(f"{key} seed {seed}: qn_inkernel_waves {st['qn_inkernel_waves']} qn_batches {st['qn_batches']} "
              f"bubbles_fused {st['bubbles_fused']} regime {_regime(st)}; rows vs the oracle's: KL rel err "
              f"{_rel(da[:, 0], oa[:, 0]):.2e}, largest abs err of any entry {np.abs(da - oa).max():.2e}")
        for r, q in zip(rows, orows):
            for a, b in zip(r[:5], q[:5]):
                assert _close(a, b, rel=1e-8, atol=1e-11), (r, q)
        dx, ox = dict(zip(dn, lrn.x())), dict(zip(on, o.x()))
        for k in dx:
            assert _close(dx[k], ox[k], rel=1e-8, atol=1e-10), k
        if not rmin:
            continue
        got = np.array(rows)[:, 5]
        print(f"{key} seed {seed}: rmin column rel err on the trajectory {_rel(got, want_rmin):.2e}")
        np.testing.assert_allclose(got, want_rmin, rtol=1e-8)
        # the oracle's own answer to where the minimum lies at the device's x
        x3 = dict(zip(dn, lrn.x()))
        want, rpp, mrow = B.oracle_rmin(o, np.array([x3[n] for n in on]))
        holders = {s for s in range(len(mrow) - 1) if mrow[s + 1] - mrow[s] > 1 and rpp[mrow[s]:mrow[s + 1]].min() == want}
        min_on_multi.append(all(n_bub[s] > 1 for s in holders))
        _, s = _check_rmin_row(key, lrn, o, on, dn)
        assert s in holders or abs(rpp[mrow[s]:mrow[s + 1]].min() - want) <= 1e-12 * want
    if rmin:
        assert any(min_on_multi), "no draw has its smallest relative path probability on a string of several bubbles"
    st = lrn.stats()
    if key == "mixed":
        assert st["stream_delta"] == 1
    if not inkernel:
        assert st["qn_inkernel_waves"] == 0
    elif st["stream_delta"] == 1 and (st["bubbles_fused"] == 1 or not rmin):
        # (the rmin column rides in the stream kernel only with the bubbles fused into it)
        assert st["qn_inkernel_waves"] > 0 and st["qn_batches"] > 0, "the in-kernel update did not run"


# -- lane groups -----------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 129])
def test_lane_groups(n, monkeypatch):
    """n identical class-A bubbles and n identical class-B bubbles in
    distinct strings of distinct weights: whole butterfly groups, leftover
    lanes beside them and a partial last wave, the runs starting at lane 3 of
    their lists.  The gradient and log q against the oracle with the slot
    merge and without it; for n >= 64 the merge saves contribution chunks;
    the default against WFSA_BUBBLE_SHAPES=0 bit for bit"""
    c = B.lanes(n)
    assert len(np.unique(c.wt)) == len(c.wt)
    # the three d2 bubbles sort before the d2b run: every H -> d2 parameter is numbered first
    first = {g: [j for j, (s, k, l) in enumerate(_fsa(n).param_names()) if s == "H" and l.startswith(g + "_")]
             for g in B.LANES_FIRST}
    assert len(first["d2"]) == len(first["d2b"]) == 2 and max(first["d2"]) < min(first["d2b"])
    merged = _learner(n, monkeypatch)
    plain = _learner(n, monkeypatch, {"WFSA_SLOT_MERGE": "0"})
    generic = _learner(n, monkeypatch, {"WFSA_BUBBLE_SHAPES": "0"})
    want = c.expected()
    sm, sp = merged.stats(), plain.stats()
    print(f"lanes {n}: class A {sm['small_bubbles_a']} class B {sm['small_bubbles_b']} big {sm['big_bubbles']} "
          f"slot_chunks merged {sm['slot_chunks']} unmerged {sp['slot_chunks']} regime {_regime(sm)}")
    for st in (sm, sp):
        assert {k: st[k] for k in COUNTERS} == want
    assert (want["small_bubbles_a"], want["small_bubbles_b"]) == (n + 4, n + 4)
    if n >= 64:
        assert sm["slot_chunks"] < sp["slot_chunks"]
    for seed in B.SEEDS:
        _check_evaluation(n, merged, seed, "merged")
        _check_evaluation(n, plain, seed, "unmerged")
        _perturb(merged, n, seed)
        _perturb(generic, n, seed)
        for want_logq in (False, True):
            kl_a, g_a, lq_a = merged.objective_grad(want_logq=want_logq)
            kl_b, g_b, lq_b = generic.objective_grad(want_logq=want_logq)
            assert kl_a == kl_b, (want_logq, kl_a, kl_b)
            assert np.array_equal(g_a, g_b), (want_logq, np.flatnonzero(g_a != g_b)[:8])
            if want_logq:
                assert np.array_equal(lq_a, lq_b), np.flatnonzero(lq_a != lq_b)[:8]
    assert generic.stats()["shaped_bubbles"] == 0 and sm["shaped_bubbles"] == 2 * n + 8


# -- reproducibility ---------------------------------------------------------------

def _evaluate(lrn):
    kl, g, _ = lrn.objective_grad()
    kl2, g2, logq = lrn.objective_grad(want_logq=True)
    return kl, g, kl2, g2, logq


def _assert_same_bits(u, v):
    assert u[0] == v[0] and u[2] == v[2]
    np.testing.assert_array_equal(u[1], v[1])
    np.testing.assert_array_equal(u[3], v[3])
    np.testing.assert_array_equal(u[4], v[4])


def test_evaluations_are_bitwise_reproducible(monkeypatch):
    """the all-gadget corpus twice in one context and once in a fresh one:
    KL, the gradient and log q with equal bits (as
    test_gpu_regimes.test_evaluations_are_bitwise_reproducible)"""
    lrn = _learner("all", monkeypatch)
    _perturb(lrn, "all", B.SEEDS[0])
    first, second = _evaluate(lrn), _evaluate(lrn)
    _assert_same_bits(first, second)
    other = _learner("all", monkeypatch)
    _perturb(other, "all", B.SEEDS[0])
    _assert_same_bits(first, _evaluate(other))
