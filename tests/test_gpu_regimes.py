"""The per-iteration path's regimes beyond c3's parameter count.

The host picks the stream kernel's variant and launch geometry from the
automaton's parameter count n_full and a few structural counts
(w-fsa_amd/csrc/wfsa_dev.hip): 512- or 1024-thread blocks, the
weight table staged in LDS or read from global memory, 16- or 32-bit stream
words, multi-parameter composites, the delta format, the bubbles fused into
the stream kernel or a launch of their own, the preparation-time gradient in
LDS or in per-block slabs.  The families below sit on both sides of each
threshold; stats() says which regime ran, and every family is compared with
the reference algorithm restated (the ENUM oracle: BFS path enumeration + the
P/M SpMV chain, src/Learner.cpp:276-348,515-553,
src/QuasiNewtonLearner.cpp:93-125,162-201).

Each corpus is 6000 walks of the automaton (the ones longer than 3 symbols)
plus 200 walks of at most 3 symbols over the same automaton: a string of 2-4
trivial words over a 10k-30k slot table needs bridging steps onto zero slots,
its delta row is header-only and its last words end on the table's end slot.

fbs_kernel<WIDE=true, W_LDS=true, MULTI=false> is not reachable: wide words
without composites need 32,768 parameters, whose table does not fit in LDS.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


# id: (n_states, degree, emissions), n_full, the regime stats() must report.
# The block / table boundaries follow from delta_table() (fb_kernels.hpp) and
# kLdsPerCu - 1024 = 162,816 bytes: two staged tables fit up to n_full 10,151,
# one up to 20,303; the words go wide at n_full 0x8000 or 0x7fff composites.
FAMILIES = {
    "block512_last": ((1127, 8, 1), 10_151, dict(stream_block=512, stream_w_lds=1, stream_delta=1)),
    "block1024_first": ((1128, 8, 1), 10_160, dict(stream_block=1024, stream_w_lds=1, stream_delta=1)),
    "lds_last": ((2255, 8, 1), 20_303, dict(stream_block=1024, stream_w_lds=1, stream_delta=1, grad_tables=1)),
    "lds_first_out": ((2256, 8, 1), 20_312, dict(stream_w_lds=0, stream_delta=0, stream_wide=0)),
    "narrow_last": ((4095, 7, 1), 32_767, dict(stream_w_lds=0, stream_wide=0, grad_tables=0)),
    "wide_first": ((3640, 8, 1), 32_768, dict(stream_w_lds=0, stream_wide=1)),
    "lds_multi": ((1000, 8, 2), 11_008, dict(stream_w_lds=1, stream_multi=1, stream_wide=0)),
    "nolds_multi": ((2000, 8, 2), 22_008, dict(stream_w_lds=0, stream_multi=1, stream_wide=0)),
    "wide_lds_multi": ((1400, 8, 3), 16_808, dict(stream_w_lds=1, stream_multi=1, stream_wide=1)),
    "wide_nolds_multi": ((3000, 8, 2), 33_008, dict(stream_w_lds=0, stream_multi=1, stream_wide=1)),
}
DELTA = ["block512_last", "block1024_first", "lds_last"]   # the families on the delta format
# traversal strings (every string ambiguous enough to leave the compiled
# stream) over more parameters than the wave kernels' LDS gradient table holds
TRAVERSAL = {"trav_26k": (2000, 26_008), "trav_wide": (2600, 33_808)}


@pytest.fixture(scope="module", autouse=True)
def _drop_caches():
    """the families and references are shared by this module's tests only"""
    yield
    for cached in (_family, _reference, _prepared_stats):
        cached.cache_clear()


def _close(a, b, rel, atol=1e-13):
    return abs(a - b) <= max(atol, rel * max(abs(a), abs(b)))


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = np.maximum(np.abs(a), np.abs(b))
    return float(np.max(np.where(d > 0, np.abs(a - b) / np.where(d > 0, d, 1.0), 0.0))) if a.size else 0.0


class _Family:
    def __init__(self, text, sym, off, wt):
        import wfsa_amd as W
        self.text, self.sym, self.off, self.wt = text, sym, off, wt
        self.fsa = W.Fsa.read_text(text)
        self.n_full = len(self.fsa.param_names())

    def oracle(self):
        from oracle import ENUM, Oracle
        return Oracle.from_arrays(self.text, self.sym, self.off, self.wt, mode=ENUM, max_paths=10_000_000)

    def learner(self, rmin=False):
        import wfsa_amd as W
        lrn = W.QuasiNewtonLearner(0)
        lrn.set_info_rmin(rmin)
        lrn.BuildFromPacked(self.fsa, self.sym, self.off, self.wt)
        lrn.Finalize()
        lrn.Init(7)
        return lrn


@functools.lru_cache(maxsize=None)
def _family(fid):
    import wfsa_amd as W
    if fid in TRAVERSAL:
        syn = W.Synthetic(seed=11, n_states=TRAVERSAL[fid][0], degree=8, vocab=16, emissions=4, n_strings=300,
                          max_len=12)
        return _Family(syn.wfsa_text, *syn.corpus())
    n_states, degree, emissions = FAMILIES[fid][0]
    shape = dict(seed=11, vocab=64, n_states=n_states, degree=degree, emissions=emissions)
    long_, short = W.Synthetic(n_strings=6000, max_len=128, **shape), W.Synthetic(n_strings=200, max_len=3, **shape)
    # the generator draws the automaton before the strings: one automaton
    assert long_.wfsa_text == short.wfsa_text
    sym_l, off_l, wt_l = long_.corpus()
    sym_s, off_s, wt_s = short.corpus()
    len_l, len_s = np.diff(off_l), np.diff(off_s)
    assert len_s.max() <= 3 and len_s.min() >= 1
    keep = np.flatnonzero(len_l > 3)   # (a long walk of <= 3 symbols may repeat a short one)
    sym = np.concatenate([sym_l[off_l[i]:off_l[i + 1]] for i in keep] + [sym_s]).astype(np.uint8)
    off = np.concatenate([[0], np.cumsum(np.concatenate([len_l[keep], len_s]))]).astype(np.int64)
    strings = {bytes(sym[off[i]:off[i + 1]]) for i in range(len(off) - 1)}
    assert len(strings) == len(off) - 1
    return _Family(long_.wfsa_text, sym, off, np.concatenate([wt_l[keep], wt_s]))


def _perturbation(names):
    """the same move off the initial point for the learner and the oracle:
    rng.normal(0, 0.5) per trimmed parameter, by name"""
    keys = sorted(names)
    return dict(zip(keys, np.random.default_rng(5).normal(0.0, 0.5, size=len(keys))))


@functools.lru_cache(maxsize=None)
def _reference(fid):
    """the ENUM oracle's evaluation at the perturbed point, computed once:
    (names, step by name, KL, gradient by name, log q per string)"""
    o = _family(fid).oracle()
    o.qn_init(7)
    names = o.param_names()
    step = _perturbation(names)
    o.set_x(o.x() + np.array([step[n] for n in names]))
    kl, _ = o.objective_grad()
    grad, logq = dict(zip(names, o.grad())), o.logq()
    grad_arr = np.array([grad[n] for n in sorted(grad)])
    grad_arr.setflags(write=False)
    logq.setflags(write=False)
    return tuple(names), step, kl, grad_arr, logq


def _perturb(lrn, fid):
    names, step, *_ = _reference(fid)
    dn = lrn.param_names()
    assert sorted(dn) == sorted(names)
    lrn.set_x(lrn.x() + np.array([step[n] for n in dn]))
    return dn


def _check_regime(fid, st):
    fam = _family(fid)
    assert fam.n_full == FAMILIES[fid][1]
    got = {k: st[k] for k in FAMILIES[fid][2]}
    assert got == FAMILIES[fid][2], f"{fid}: regime {_regime(st)}"
    assert st["stream_block"] in (512, 1024)
    assert st["stream_delta"] <= st["stream_w_lds"]          # the delta format needs the staged table
    assert st["bubbles_fused"] <= st["stream_w_lds"]
    assert st["compiled_strings"] > 0.95 * len(fam.wt) and st["n_bubbles"] > 0


REGIME_KEYS = ("stream_block", "stream_w_lds", "stream_wide", "stream_multi", "stream_delta", "bubbles_fused",
               "grad_tables", "wave_lgrad")


def _regime(st):
    return {k: st[k] for k in REGIME_KEYS}


@functools.lru_cache(maxsize=None)
def _prepared_stats(fid):
    return _family(fid).learner().stats()


@pytest.mark.parametrize("fid", list(FAMILIES))
def test_family_runs_its_regime(fid):
    """n_full as the table says, and stats() on the intended side of each
    threshold (the pairs straddle: block512_last / block1024_first,
    lds_last / lds_first_out, narrow_last / wide_first)"""
    st = _prepared_stats(fid)
    print(f"{fid}: n_full {_family(fid).n_full} regime {_regime(st)} compiled {st['compiled_strings']} "
          f"bubbles {st['n_bubbles']} fallback {st['fallback_strings']}")
    _check_regime(fid, st)


def test_families_cover_every_switch():
    """both block sizes; 0 and 1 of every other switch; the seven reachable
    (wide, w_lds, multi) stream kernels"""
    sts = [_prepared_stats(fid) for fid in FAMILIES]
    assert {st["stream_block"] for st in sts} == {512, 1024}
    for k in ("stream_w_lds", "stream_wide", "stream_multi", "stream_delta", "grad_tables"):
        assert {st[k] for st in sts} == {0, 1}, k
    combos = {(st["stream_wide"], st["stream_w_lds"], st["stream_multi"]) for st in sts}
    assert combos == {(w, t, m) for w in (0, 1) for t in (0, 1) for m in (0, 1)} - {(1, 1, 0)}


def _check_evaluation(fid, lrn, rtol_logq=1e-12, atol_logq=1e-12, rel_kl=1e-11, rtol_g=1e-10):
    """KL and the gradient from objective_grad() (bubbles fused where the
    regime allows, the reduction kernel), log q of every string from
    objective_grad(want_logq=True) (bubbles unfused), against ENUM at the
    perturbed point"""
    names, _, kl_o, g_o, logq_o = _reference(fid)
    dn = _perturb(lrn, fid)
    kl, g, _ = lrn.objective_grad()
    kl2, g2, logq = lrn.objective_grad(want_logq=True)
    by, by2 = dict(zip(dn, g)), dict(zip(dn, g2))
    keys = sorted(by)   # (_reference's order)
    g_d, g2_d = np.array([by[k] for k in keys]), np.array([by2[k] for k in keys])
    print(f"{fid}: rel err vs ENUM: KL {abs(kl - kl_o) / abs(kl_o):.2e} grad {_rel(g_d, g_o):.2e} "
          f"(abs {np.abs(g_d - g_o).max():.2e}) logq {_rel(logq, logq_o):.2e}; with logq: KL "
          f"{abs(kl2 - kl_o) / abs(kl_o):.2e} grad {_rel(g2_d, g_o):.2e}")
    assert np.isfinite(logq_o).all() and np.isfinite(g_o).all()
    assert _close(kl, kl_o, rel=rel_kl)
    np.testing.assert_allclose(g_d, g_o, rtol=rtol_g, atol=1e-15)
    np.testing.assert_allclose(logq, logq_o, rtol=rtol_logq, atol=atol_logq)
    assert _close(kl2, kl_o, rel=rel_kl)
    np.testing.assert_allclose(g2_d, g_o, rtol=rtol_g, atol=1e-15)


@pytest.mark.parametrize("fid", list(FAMILIES))
def test_evaluation_matches_enum(fid):
    lrn = _family(fid).learner()
    _check_regime(fid, lrn.stats())
    _check_evaluation(fid, lrn)


def _oracle_rmin(o, x):
    """(smallest relative path probability over the ambiguous strings' paths,
    relative path probabilities, M's row pointers) at x, from the path
    matrices (ComputeModeledProbs, src/Learner.cpp:515-547)"""
    prow, pcol, pdata, mrow = o.paths()
    path = np.repeat(np.arange(len(prow) - 1), np.diff(prow))
    lw = np.bincount(path, weights=pdata * x[pcol], minlength=len(prow) - 1)
    n_p = np.diff(mrow)
    assert n_p.min() >= 1
    e = np.exp(lw - np.repeat(np.maximum.reduceat(lw, mrow[:-1]), n_p))
    rpp = e / np.repeat(np.add.reduceat(e, mrow[:-1]), n_p)
    amb = np.where(np.repeat(n_p > 1, n_p), rpp, np.inf)
    return float(amb.min()), rpp, mrow


@pytest.mark.parametrize("rmin", [False, True], ids=["", "rmin"])
@pytest.mark.parametrize("fid", list(FAMILIES))
def test_device_qn_loop_matches_oracle_steps(fid, rmin):
    """six device-resident steps against six of the oracle's; with the rmin
    column on, the column on the oracle's trajectory and -- one step more --
    at exactly the device's weights"""
    fam = _family(fid)
    lrn = fam.learner(rmin)
    _check_regime(fid, lrn.stats())
    o = fam.oracle()
    o.qn_init(7)
    dn, on = lrn.param_names(), o.param_names()
    assert sorted(dn) == sorted(on)
    want_rmin, orows = [], []
    for _ in range(6):
        if rmin:
            want_rmin.append(_oracle_rmin(o, o.x())[0])
        orows.append(o.qn_step(1.0))
    rows = lrn.Run(6, 1.0, -1.0)
    assert len(rows) == 6
    st = lrn.stats()
    print(f"{fid}: qn_inkernel_waves {st['qn_inkernel_waves']} qn_batches {st['qn_batches']} regime {_regime(st)}")
    da, oa = np.array(rows)[:, :5], np.array(orows)[:, :5]
    print(f"{fid}: info rows vs the oracle's: KL rel err {_rel(da[:, 0], oa[:, 0]):.2e}, "
          f"largest abs err of any entry {np.abs(da - oa).max():.2e}")
    for r, q in zip(rows, orows):
        for a, b in zip(r[:5], q[:5]):
            assert _close(a, b, rel=1e-8, atol=1e-11), (r, q)
    dx, ox = dict(zip(dn, lrn.x())), dict(zip(on, o.x()))
    for k in dx:
        assert _close(dx[k], ox[k], rel=1e-8, atol=1e-10), k
    if not rmin:
        return
    # on the oracle's trajectory: the steps' own tolerance
    got = np.array(rows)[:, 5]
    print(f"{fid}: rmin column rel err on the trajectory {_rel(got, want_rmin):.2e}")
    np.testing.assert_allclose(got, want_rmin, rtol=1e-8)
    # at the same weights: row 6 is evaluated at the x the run left
    x6 = dict(zip(dn, lrn.x()))
    row = lrn.Run(1, 1.0, -1.0)[0]
    want, rpp, mrow = _oracle_rmin(o, np.array([x6[n] for n in on]))
    print(f"{fid}: rmin {row[5]:.17g} want {want:.17g} rel err {abs(row[5] - want) / want:.2e} string {int(row[6])}")
    assert abs(row[5] - want) <= 1e-12 * want, (row[5], want)
    s = int(row[6])
    assert 0 <= s < len(mrow) - 1 and mrow[s + 1] - mrow[s] > 1   # an ambiguous string holding that minimum
    assert abs(rpp[mrow[s]:mrow[s + 1]].min() - want) <= 1e-12 * want


def _inkernel_learner(fam, monkeypatch, inkernel, rmin):
    monkeypatch.setenv("WFSA_QN_INKERNEL", "1" if inkernel else "0")
    monkeypatch.setenv("WFSA_QN_LAST_SELF", "1")
    return fam.learner(rmin)


@pytest.mark.parametrize("rmin", [False, True], ids=["", "rmin"])
@pytest.mark.parametrize("fid", DELTA)
def test_inkernel_update_equals_qn_step_kernel(fid, rmin, monkeypatch):
    """test_gpu_qn_inkernel.py's sequence where a few 1024-thread blocks make
    the grid: the batches far outnumber the QN waves (the kernel's
    b += q.n_waves loop), 16 waves arrive per block.  Rows, x, the last
    gradient and the next evaluation equal the separate kernel's bit for bit"""
    fam = _family(fid)
    a = _inkernel_learner(fam, monkeypatch, True, rmin)
    b = _inkernel_learner(fam, monkeypatch, False, rmin)
    st0 = a.stats()
    _check_regime(fid, st0)
    assert st0["stream_delta"] == 1
    r1a, r1b = a.Run(1, 1.0, -1.0), b.Run(1, 1.0, -1.0)
    np.testing.assert_array_equal(a.last_grad(), b.last_grad())
    np.testing.assert_array_equal(a.x(), b.x())
    np.testing.assert_array_equal(np.array(r1a), np.array(r1b))
    a.Init(7)
    b.Init(7)
    ra = a.Run(3, 1.0, -1.0) + a.Run(4, 1.0, -1.0) + a.Run(1, 1.0, -1.0) + a.Run(12, 1.0, -1.0)
    sa = a.stats()
    rb = b.Run(20, 1.0, -1.0)
    print(f"{fid}: bubbles_fused {sa['bubbles_fused']} qn_inkernel_waves {sa['qn_inkernel_waves']} "
          f"qn_batches {sa['qn_batches']}")
    if sa["bubbles_fused"] == 1 or not rmin:
        assert sa["qn_inkernel_waves"] > 0 and sa["qn_batches"] > 0, "the in-kernel update did not run"
        assert sa["qn_batches"] > sa["qn_inkernel_waves"]   # several batches per QN wave
    else:   # the rmin column rides in the stream kernel only with the bubbles fused into it
        assert sa["qn_inkernel_waves"] == 0
    assert b.stats()["qn_inkernel_waves"] == 0
    ra, rb = np.array(ra), np.array(rb)
    assert ra.shape == rb.shape == (20, ra.shape[1])
    if rmin:
        assert (ra[:, 6] >= 0).all() and (ra[:, 5] > 0).all(), ra[:, 5:7]
    bad = sorted(set(int(r) for r, _ in np.argwhere(ra != rb)))
    assert not bad, f"rows {bad} differ: {ra[bad].tolist()} vs {rb[bad].tolist()}"
    np.testing.assert_array_equal(a.x(), b.x())
    np.testing.assert_array_equal(a.last_grad(), b.last_grad())
    kl_a, g_a, _ = a.objective_grad()
    kl_b, g_b, _ = b.objective_grad()
    assert kl_a == kl_b and np.array_equal(g_a, g_b)


def _evaluate(lrn):
    kl, g, _ = lrn.objective_grad()
    kl2, g2, logq = lrn.objective_grad(want_logq=True)
    return kl, g, kl2, g2, logq


def _assert_same_bits(u, v, logq):
    """KL and the gradient of both evaluations (logq False), or log q (True)"""
    if logq:
        diff = np.flatnonzero(u[4] != v[4])
        print(f"log q: {len(diff)} of {len(u[4])} strings differ, worst "
              f"{_rel(u[4][diff], v[4][diff]):.2e} relative")
        np.testing.assert_array_equal(u[4], v[4])
        return
    assert u[0] == v[0] and u[2] == v[2]
    np.testing.assert_array_equal(u[1], v[1])
    np.testing.assert_array_equal(u[3], v[3])


@pytest.mark.parametrize("what", ["kl_grad", "logq"])
@pytest.mark.parametrize("fid", list(FAMILIES))
def test_evaluations_are_bitwise_reproducible(fid, what):
    """the same evaluation twice in one context, and once in a fresh context
    (a fresh compilation, fresh buffers): equal bits for KL and the gradient
    (kl_grad: without and with log q wanted) and for log q.
    With log q wanted the bubbles run in bubble_kernel, which stores each
    bubble's log Z at its list position; logq_bubbles_kernel adds them to
    the stream kernel's sum per string in bubble order (they used to be
    added with floating-point atomics, in whatever order those landed: one
    ulp of difference in a few strings with two or more bubbles)."""
    lrn = _family(fid).learner()
    _perturb(lrn, fid)
    first, second = _evaluate(lrn), _evaluate(lrn)
    _assert_same_bits(first, second, what == "logq")
    other = _family(fid).learner()
    _perturb(other, fid)
    _assert_same_bits(first, _evaluate(other), what == "logq")


def _dirty_device_memory(gib=8):
    """hipMalloc'd, filled with 0xff bytes (NaN doubles) and freed again, in
    the HIP runtime the library uses, so its next allocations are likely
    handed these pages (as tests/test_gpu_parity.py)"""
    import ctypes
    import wfsa_amd as W
    W.Device(0)   # the library's HIP runtime up
    libs = sorted({ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln})
    assert libs
    hip = ctypes.CDLL(libs[0]) if len(libs) == 1 else ctypes.CDLL("libamdhip64.so.7")
    ptrs = []
    for _ in range(gib):
        p = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(1 << 30)) == 0
        assert hip.hipMemset(p, 0xff, ctypes.c_size_t(1 << 30)) == 0
        ptrs.append(p)
    assert hip.hipDeviceSynchronize() == 0
    for p in ptrs:
        assert hip.hipFree(p) == 0


@pytest.mark.parametrize("fid", ["lds_first_out", "wide_first"])
def test_evaluation_on_dirty_device_memory(fid):
    """the gradient slabs, lw / ew / erec and the wide stream are buffers of
    the regimes without the staged table: none may rely on hipMalloc
    returning zeros"""
    _dirty_device_memory()
    lrn = _family(fid).learner()
    st = lrn.stats()
    _check_regime(fid, st)
    assert st["stream_w_lds"] == 0
    _check_evaluation(fid, lrn)


@pytest.mark.parametrize("fid", list(TRAVERSAL))
def test_traversal_strings_beyond_the_lds_gradient_table(fid):
    """ambiguous strings (4 of 16 symbols per state) run on the wave kernel;
    with 26k / 34k parameters its gradient table does not fit in LDS beside
    four waves (wide2_config), so the waves add into the global fixed-point
    accumulators (fix128_add: integer adds, any order gives the same sum) --
    log q and the gradient against ENUM at test_gpu_tier2.py's tolerances,
    and equal bits from a second evaluation"""
    fam = _family(fid)
    assert fam.n_full == TRAVERSAL[fid][1]
    lrn = fam.learner()
    st = lrn.stats()
    print(f"{fid}: fallback {st['fallback_strings']} wave_strings {st['wave_strings']} wave_lgrad {st['wave_lgrad']} "
          f"wave_pull {st['wave_pull']} tier2 {st['tier2_strings']} compiled {st['compiled_strings']}")
    assert st["fallback_strings"] > 0
    # a wave-kernel configuration always exists (four waves' rows without the
    # table fit in LDS): every traversal string is on it, the table is not in LDS
    # (wave_pull 0 here: a D(b) of more than 512 nodes leaves the pull layout
    # out, wide2_kernel pushes -- the same fixed-point sums)
    assert st["wave_lgrad"] == 0 and st["wave_strings"] == st["fallback_strings"]
    # (the few strings that compile: 4 emissions per state make more than 0x7fff composite edges)
    assert st["stream_wide"] == 1 and st["stream_multi"] == 1
    _check_evaluation(fid, lrn, rtol_logq=1e-11, atol_logq=0.0, rel_kl=1e-11, rtol_g=1e-9)
    _assert_same_bits(_evaluate(lrn), _evaluate(lrn), False)
