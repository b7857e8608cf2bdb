"""The traversal kernels on automata built by hand (traversal_gadgets.py):
composite edges, the D(b) steps of the pull layout and the slab capacities.

The other traversal tests draw their automata from Synthetic(...): single-byte
emissions, no epsilon, one end transition per state -- one or two parameters
per trellis edge, and sizes that are an accident of a seed.  Here

  * the composite automaton (edges of up to six parameters, parallel edges,
    chain nodes of multi-byte emissions, several composite end edges per node
    or none) and the golden fixtures run on wave_pull_kernel, wide2_kernel,
    wide_kernel and, the composite one, trav_kernel<MODE_WEIGHTED>;
  * the D(b) family sits on both sides of every step of build_pull_tables'
    lanes-per-item rule, with the gradient table in LDS and without it;
  * the capacity family holds strings one under, at and one over each of the
    four slab capacities.

Every route is confirmed from stats().  log q, the log-likelihood and the
gradient are held to the TRELLIS oracle at test_gpu_tier2's tolerances (log q
rtol 1e-11, log-likelihood relative 1e-11, gradient rtol 1e-9 atol 1e-15; pull
against push 1e-12 / 1e-10); test_traversal_gadgets_reference.py shows that
the oracle itself is inside them.  No string and no parameter is left out of
a comparison; the two rejected strings of the composite corpus have log q
-inf and make the log-likelihood -inf.  Each test prints its worst relative
errors (profiles/traversal_gadgets/errors.json).  Needs a gfx950 device."""
import os

import numpy as np
import pytest

import bubble_gadgets as B
import traversal_gadgets as T
from conftest import DATA

pytestmark = pytest.mark.gpu

TIER2_ROUTES = ("pull", "push", "wide")


@pytest.fixture(scope="module", autouse=True)
def _drop_caches():
    """the corpora and references are shared by this module's tests only"""
    yield
    for cached in (T.composite, T.db, T.capacity, _corpus, _reference, _enum):
        cached.cache_clear()


def _close(a, b, rel, atol=1e-13):
    return abs(a - b) <= max(atol, rel * max(abs(a), abs(b)))


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = np.maximum(np.abs(a), np.abs(b))
    return float(np.max(np.where(d > 0, np.abs(a - b) / np.where(d > 0, d, 1.0), 0.0))) if a.size else 0.0


def _memo(fn):
    cache = {}

    def wrapped(*key):
        if key not in cache:
            cache[key] = fn(*key)
        return cache[key]
    wrapped.cache_clear = cache.clear
    return wrapped


class Packed:
    """a corpus as the device and the oracles take it"""

    def __init__(self, text, sym, off, wt):
        self.text, self.sym, self.off, self.wt = text, np.asarray(sym), np.asarray(off), np.asarray(wt, dtype=np.float64)

    def __len__(self):
        return len(self.wt)

    def subset(self, mask):
        keep = np.flatnonzero(mask)
        strings = [bytes(self.sym[self.off[i]:self.off[i + 1]]) for i in keep]
        sym = np.frombuffer(b"".join(strings), dtype=np.uint8).copy()
        off = np.concatenate([[0], np.cumsum([len(s) for s in strings])]).astype(np.int64)
        return Packed(self.text, sym, off, self.wt[keep])


def _golden(wfsa, corpus):
    import wfsa_amd as W
    text = open(os.path.join(DATA, wfsa + ".wfsa"), "rb").read().decode("latin-1")
    return Packed(text, *W.Corpus.read_file(os.path.join(DATA, corpus + ".corpus")).packed())


@_memo
def _corpus(key):
    """composite / ("db", w1, w2) / capacity / ("golden", wfsa, corpus)"""
    if key == "composite":
        c = T.composite()
    elif key == "capacity":
        c = T.capacity()[0]
    elif key[0] == "db":
        c = T.db(*key[1:])
    else:
        return _golden(*key[1:])
    return Packed(c.text, c.sym, c.off, c.wt)


@_memo
def _enum(key):
    """(path counts, used parameter names, the ENUM oracle of the recognized strings)"""
    from oracle import ENUM, Oracle
    c = _corpus(key)
    o = Oracle.from_arrays(c.text, c.sym, c.off, c.wt, mode=ENUM, max_paths=10_000_000)
    pc = o.path_counts().astype(np.float64)
    used = {n for n, t in zip(o.full_param_names(), o.trimmed_index()) if t != -2}
    if not (pc > 0).all():
        k = c.subset(pc > 0)
        o = Oracle.from_arrays(k.text, k.sym, k.off, k.wt, mode=ENUM, max_paths=10_000_000)
    return pc, used, o


@_memo
def _reference(key, recognized, seed):
    """the TRELLIS oracle over the recognized strings at weights(seed), computed once and left unchanged"""
    c = _corpus(key)
    return T.trellis_reference(c.subset(np.array(recognized)), seed)


ERRORS = {}


def _note(family, route, **errs):
    worst = ERRORS.setdefault((family, route), {})
    for k, v in errs.items():
        worst[k] = max(worst.get(k, 0.0), v)
    print(f"traversal_gadgets worst rel err | {family} | {route} | " + " ".join(f"{k} {v:.3e}" for k, v in sorted(worst.items())))


def _device(key, route, monkeypatch):
    import wfsa_amd as W
    T.set_route(monkeypatch, route)
    fsa = W.Fsa.read_text(_corpus(key).text)
    dev = W.Device(0)
    dev.load_model(fsa)
    return dev, fsa.param_names()


def _load(dev, c):
    dev.load_corpus(c.sym, c.off, c.wt / c.wt.sum())
    return dev.recognize()


def _evaluate(key, route, monkeypatch, want_pc, family, want_used=None, n_traversal=None, confirm=True):
    """Loads the corpus on the route and checks recognized, the path counts
    and the used set; with rejected strings in the corpus, that they have log
    q -inf and make the log-likelihood -inf while every other log q is the
    oracle's; then, on the recognized strings, log q, the log-likelihood and
    the gradient against TRELLIS at every seed.  Returns the device (the
    recognized strings loaded), the names, stats() and the last seed's
    (weights, ll, gradient, log q)"""
    c = _corpus(key)
    want_pc = np.asarray(want_pc, dtype=np.float64)
    rec_o = want_pc > 0
    dev, names = _device(key, route, monkeypatch)
    rec, pc, used = _load(dev, c)
    np.testing.assert_array_equal(rec.astype(bool), rec_o)
    np.testing.assert_array_equal(pc, want_pc)
    if want_used is not None:
        assert {n for n, u in zip(names, used) if u} == want_used
    clean = c if rec_o.all() else c.subset(rec_o)
    out = None
    for seed in T.SEEDS:
        w_by, ll_o, logq_o, grad_o = _reference(key, tuple(rec_o), seed)
        assert sorted(w_by) == sorted(names)
        w = np.array([w_by[n] for n in names])
        g_o = np.array([grad_o[n] for n in names])
        if not rec_o.all():
            _load(dev, c)
            ll, _, logq = dev.objective_grad(w)
            if confirm:   # (stats() knows the route once an evaluation has prepared the corpus)
                T.confirm_route(route, dev.stats(), len(c), len(c) if n_traversal is None else n_traversal)
            assert ll == -np.inf, ll
            assert (logq[~rec_o] == -np.inf).all(), logq[~rec_o]
            np.testing.assert_allclose(logq[rec_o], logq_o, rtol=1e-11)
            rec2, pc2, _ = _load(dev, clean)
            assert rec2.all() and np.array_equal(pc2, want_pc[rec_o])
        ll, grad, logq = dev.objective_grad(w)
        if confirm and rec_o.all():
            T.confirm_route(route, dev.stats(), len(c), len(c) if n_traversal is None else n_traversal)
        assert np.isfinite(logq_o).all() and np.isfinite(g_o).all() and logq.shape == logq_o.shape
        _note(family, route, logq=_rel(logq, logq_o), ll=abs(ll - ll_o) / abs(ll_o), grad=_rel(grad, g_o),
              grad_abs=float(np.abs(grad - g_o).max()))
        np.testing.assert_allclose(logq, logq_o, rtol=1e-11)
        assert _close(ll, ll_o, rel=1e-11), (ll, ll_o)
        np.testing.assert_allclose(grad, g_o, rtol=1e-9, atol=1e-15)
        out = (w, ll, grad, logq)
    return dev, names, dev.stats(), out


def _check_rmin(key, dev, names, w):
    """the rmin column of the weighted pass (the kernels' TRACK instantiations)
    against the oracle's enumerated paths, as test_gpu_rmin._check"""
    o = _enum(key)[2]
    w_by = dict(zip(names, w))
    x = np.array([w_by[n] for n in o.param_names()])
    want, rpp, mrow = B.oracle_rmin(o, x)
    # the oracle's own weights at x (a parameter no recognized string uses: -inf), as test_gpu_rmin._setup
    o.set_x(x)
    w_full = dict(zip(o.full_param_names(), o.w_full()))
    dev.objective_grad(np.array([w_full[n] for n in names]), want_logq=False)
    r, s = dev.rmin()
    if not np.isfinite(want):   # no ambiguous string
        assert s == -1
        return
    print(f"{key}: rmin {r:.17g} want {want:.17g} rel err {abs(r - want) / want:.2e} string {s}")
    assert abs(r - want) <= 1e-12 * want, (r, want)
    assert 0 <= s < len(mrow) - 1 and mrow[s + 1] - mrow[s] > 1
    assert abs(rpp[mrow[s]:mrow[s + 1]].min() - want) <= 1e-12 * want


def _assert_repeats(dev, w, first):
    ll, grad, logq = dev.objective_grad(w)
    assert ll == first[1] and np.array_equal(grad, first[2]) and np.array_equal(logq, first[3])


# -- the composite automaton on the four routes ---------------------------------------

@pytest.mark.parametrize("route", list(T.ROUTES))
def test_composite_edges_on_every_traversal_kernel(route, monkeypatch):
    """22 strings over the epsilon part and the 33-node gadget.  On the three
    WFSA_TIER2=1 routes every string runs on the kernel; on slab the eight
    strings that visit the gadget run on trav_kernel<MODE_WEIGHTED> with the
    composite edges before, behind and between the visits"""
    c = T.composite()
    pc, used, _ = _enum("composite")
    assert np.array_equal(pc, c.path_counts())
    trav = T.composite_traversal(c)
    dev, names, st, last = _evaluate("composite", route, monkeypatch, pc, "composite", want_used=used,
                                     n_traversal=int(trav.sum()))
    # (the recognized strings are loaded now: the two rejected ones were traversal strings)
    T.confirm_route(route, st, int(c.recognized.sum()), int((trav & c.recognized).sum()))
    print(f"composite {route}: wave_strings {st['wave_strings']} wave_pull {st['wave_pull']} wave_lgrad {st['wave_lgrad']} "
          f"tier1 {st['tier1_strings']} tier2 {st['tier2_strings']} fallback {st['fallback_strings']} "
          f"compiled {st['compiled_strings']}")
    if route == "slab":
        tiers = dev.string_tiers()
        assert np.array_equal(tiers >= 0, trav[c.recognized]) and st["tier2_strings"] == 0
    else:
        _check_rmin("composite", dev, names, last[0])
    if route == "pull":
        _assert_repeats(dev, last[0], last)


# -- the golden fixtures ----------------------------------------------------------------

@pytest.mark.parametrize("route", TIER2_ROUTES)
@pytest.mark.parametrize("case", [("talk", "talk"), ("test3", "test"), ("test5", "test5"), ("test5_2", "test5"),
                                  ("test.loop", "test"), ("test.list", "test")], ids=lambda c: c[0])
def test_golden_fixtures_on_the_wave_and_wide_kernels(case, route, monkeypatch):
    """the reference project's own epsilon and multi-byte automata, every
    string forced onto the traversal kernels"""
    key = ("golden",) + case
    pc, used, _ = _enum(key)
    dev, names, st, last = _evaluate(key, route, monkeypatch, pc, "golden:" + case[0], want_used=used, confirm=False)
    T.confirm_route(route, st, int((pc > 0).sum()), int((pc > 0).sum()))
    _check_rmin(key, dev, names, last[0])
    if route == "pull":
        _assert_repeats(dev, last[0], last)


# -- the D(b) family --------------------------------------------------------------------

DB_CASES = [((T.DB_FIRST, w - T.DB_FIRST), ni, 1) for w, ni in T.DB_WIDTHS.items()] + [(T.DB_GLOBAL, 8, 0)]


@pytest.mark.parametrize("shape,items,lgrad", DB_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_pull_layout_steps(shape, items, lgrad, monkeypatch):
    """D(a) of 256, 257, 384, 385, 512 and 513 nodes: 4 items per lane with
    every lane full, then 6 (257 nodes cannot lie on 64 lanes of 4), 6 full, 8,
    8 full, and no pull layout: there wide2_kernel serves under both settings.
    (40, 472): 8 items per lane and no room for the gradient table in LDS:
    the pull kernel adds into the global fixed-point accumulators"""
    key = ("db",) + shape
    c = T.db(*shape)
    res = {}
    for route in ("pull", "push"):
        dev, names, st, last = _evaluate(key, route, monkeypatch, c.path_counts(), f"db{sum(shape)}" + ("" if lgrad else "_global"),
                                         confirm=False)
        print(f"db {shape} {route}: wave_strings {st['wave_strings']} wave_pull {st['wave_pull']} wave_lgrad {st['wave_lgrad']} "
              f"n_nodes {st['n_nodes']}")
        assert st["wave_strings"] == len(c.strings) == st["tier2_strings"]
        assert st["wave_pull"] == (items if route == "pull" else 0)
        assert st["wave_lgrad"] == lgrad
        if route == "pull":
            _assert_repeats(dev, last[0], last)
        res[route] = last
    (_, ll1, g1, lq1), (_, ll0, g0, lq0) = res["pull"], res["push"]
    np.testing.assert_allclose(lq1, lq0, rtol=1e-12)
    assert _close(ll1, ll0, rel=1e-12)
    np.testing.assert_allclose(g1, g0, rtol=1e-10, atol=1e-16)


# -- the slab capacities ------------------------------------------------------------------

def test_slab_capacities(monkeypatch):
    """strings with F or E one under, at and one over cap_f and cap_e of both
    LDS tiers: at a capacity the string stays on its tier, one entry more
    moves it up, in the count pass and in the weighted pass alike (a string
    the weighted pass dropped would miss from log q and the gradient)"""
    case, fe, caps, boundary = T.capacity()
    trav = T.capacity_traversal(case)
    dev, names, st, last = _evaluate("capacity", "slab", monkeypatch, case.path_counts(), "capacity",
                                     n_traversal=int(trav.sum()))
    assert T.slab_caps(st["max_len"], st["n_nodes"]) == caps, (st["max_len"], st["n_nodes"], caps)
    want = np.array([T.tier_of(f, e, caps) for f, e in fe])
    tiers = dev.string_tiers()
    print(f"capacity: caps {caps} max_len {st['max_len']} n_nodes {st['n_nodes']} tier1 {st['tier1_strings']} "
          f"tier2 {st['tier2_strings']} live edges {st['last_live_edges']}; (F, E, tier) of the boundary strings "
          f"{ {k: fe[i] + (int(tiers[i]),) for k, i in boundary.items()} }")
    assert st["tier1_strings"] == int((want == 1).sum()) and st["tier2_strings"] == int((want == 2).sum())
    np.testing.assert_array_equal(tiers, np.where(trav, want, -1))
    for (tier, _, delta), i in boundary.items():
        assert tiers[i] == tier + (delta == 1)
    # the count pass' live edges: trav_kernel's E on tiers 0 and 1; on tier 2 wide_kernel counts the edges its
    # forward gathers over, every edge of the position's byte
    tr = case.trellis
    gathered = [sum(tr.byte_edges(chr(b)) for b in s) for s in case.strings]
    assert st["last_live_edges"] == sum(g if t == 2 else e for (_, e), g, t in zip(fe, gathered, want))
    assert sum(e for (_, e), t in zip(fe, want) if t < 2) > 0 and (want == 2).sum() == 2
    # the same corpus on the pull kernel: the same log q whatever the tiers
    dev2, _, st2, last2 = _evaluate("capacity", "pull", monkeypatch, case.path_counts(), "capacity")
    assert st2["wave_strings"] == len(case.strings)
    np.testing.assert_allclose(last2[3], last[3], rtol=1e-12)
