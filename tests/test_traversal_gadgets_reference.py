"""The hand-built traversal cases (traversal_gadgets.py) checked without a
device: the counts the module states, its restatements of the epsilon folding
and of make_slab, the composite features its corpus claims, and the TRELLIS
oracle the GPU tests compare with against a long-double log-sum-exp over the
ENUM oracle's paths, at the GPU tests' own tolerances
(test_gpu_traversal_gadgets.py)."""
import collections

import numpy as np
import pytest

import traversal_gadgets as T

LD = np.longdouble


def _fsa(text):
    import wfsa_amd as W
    return W.Fsa.read_text(text)


def _trellis_stats(case):
    import wfsa_amd as W
    return W.trellis_stats(_fsa(case.text))


# -- hand-stated counts ----------------------------------------------------------

def test_gadget_counts_and_the_folded_trellis():
    """nodes, edges, paths per visit and D of the letter of every gadget; the
    folded trellis of every automaton has the nodes, byte edges, end edges and
    parameter-list entries the library's own compilation has, and the
    parameters are the ones the module names"""
    g = T.WIDE
    assert (g.nodes, g.edges, g.paths) == (33, 271, 240) == (33, 271, T.WIDE_PATHS)
    counts = {"u1": (3, 2, 1), "v1": (3, 2, 1), "c33": (134, 165, 33), "c34": (138, 170, 34), "c64": (514, 576, 64),
              "f1616": (34, 288, 256)}
    assert {n: (g.nodes, g.edges, g.paths) for n, g in T.CAP_GADGETS.items()} == counts
    # what a visit adds to trav_kernel's counters: mid-string with H behind it, or at the string's end
    assert T.visit_counts(T.CAP_GADGETS["u1"], False) == (2, 2, 2)
    assert T.visit_counts(T.CAP_GADGETS["c33"], False) == (133, 165, 5) and T.visit_counts(T.CAP_GADGETS["c33"], True) == (132, 132, 4)
    assert T.visit_counts(T.CAP_GADGETS["f1616"], False) == (33, 288, 3) and T.visit_counts(T.CAP_GADGETS["f1616"], True) == (32, 272, 2)
    cases = [T.composite(), T.capacity()[0], T.db(8, 248), T.db(8, 505), T.db(*T.DB_GLOBAL)]
    for c in cases:
        tr = c.trellis
        assert (len(tr.nodes), tr.n_edges, tr.n_end_edges, tr.n_entries) == _trellis_stats(c)
        assert sorted(_fsa(c.text).param_names()) == sorted(T.param_names(c.states))
    for total in T.DB_WIDTHS:
        c = T.db(T.DB_FIRST, total - T.DB_FIRST)
        tr = c.trellis
        assert len(tr.dests("a")) == total and max(len(tr.dests(b)) for b in "xu") == 1
        # the pair (a, a): every destination of the second layer has 8 in-edges, every source of the first
        # total - 8 out-edges; the first layer's nodes have no in-edge from D(a) (the empty items)
        into = collections.Counter(v for u in tr.dests("a") for b, v, _ in tr.edges[u] if b == "a")
        assert len(into) == total - 8 and set(into.values()) == {8}
        assert len(T.param_names(c.states)) == T.db_n_params(T.DB_FIRST, total - T.DB_FIRST) <= 5_100
    c = T.db(*T.DB_GLOBAL)
    assert len(c.trellis.dests("a")) == 512 and T.db_n_params(*T.DB_GLOBAL) == 19_868
    # pull_lds (fb_kernels.hpp): the gradient table beside four waves' rows of max_n doubles, in kLdsPerCu - 1024
    def pull_lds(n_params, waves, max_n):
        return ((n_params + 64 + 1) & ~1) * 8 + waves * max_n * 8
    assert pull_lds(T.db_n_params(*T.DB_GLOBAL), 4, 512) > T.TIER1_BUDGET
    assert all(pull_lds(T.db_n_params(8, w - 8), 4, w) <= T.TIER1_BUDGET for w in T.DB_WIDTHS)


def test_lanes_per_item_steps():
    """build_pull_tables' rule restated: the D(b) family sits on both sides of
    each step, and at exactly 64 NI destinations every lane holds NI items"""
    def ni(max_n):
        return 0 if max_n > 512 else 4 if max_n <= 256 else 6 if max_n <= 384 else 8
    assert {w: ni(w) for w in T.DB_WIDTHS} == T.DB_WIDTHS
    assert all(w <= 64 * n for w, n in T.DB_WIDTHS.items() if n) and all(w > 64 * (n - 2) for w, n in T.DB_WIDTHS.items() if n)
    assert [w for w in T.DB_WIDTHS if w == 64 * T.DB_WIDTHS[w]] == [256, 384, 512]


# -- path counts -----------------------------------------------------------------

def test_path_counts_equal_the_closed_forms():
    c = T.composite()
    o = T.enum_oracle(c)
    assert np.array_equal(o.path_counts(), [int(p) for p in c.paths])
    assert [T.walk(c.trellis, s)[2] for s in c.strings] == list(c.paths)
    assert list(c.recognized) == [True] * 20 + [False] * 2
    for total in (256, 257):   # ENUM stays away from the string of two wide visits (3.9M paths)
        d = T.db(T.DB_FIRST, total - T.DB_FIRST)
        small = d.subset([p <= 8 * (total - 8) for p in d.paths])
        assert len(small.strings) == len(d.strings) - 1
        assert np.array_equal(T.enum_oracle(small).path_counts(), [int(p) for p in small.paths])
        assert [T.walk(d.trellis, s)[2] for s in d.strings] == list(d.paths)
        assert list(d.paths[:4]) == [8 * (total - 8), 8 * (total - 8), (8 * (total - 8)) ** 2, 8 * (total - 8)]
    for shape in [(8, w - 8) for w in T.DB_WIDTHS] + [T.DB_GLOBAL]:
        d = T.db(*shape)
        assert T.walk(d.trellis, b"xaax")[2] == shape[0] * shape[1] and d.path_counts().max() == (shape[0] * shape[1]) ** 2


# -- the composite features ----------------------------------------------------------

def _fold_paths(tr, s):
    """every accepting path of s over the folded trellis, as the multiset of its parameters"""
    text = s.decode("latin-1")
    out = []

    def go(u, i, params):
        if i == len(text):
            out.extend(collections.Counter(params + list(p)) for p in tr.ends[u])
            return
        for b, v, p in tr.edges[u]:
            if b == text[i]:
                go(v, i + 1, params + list(p))
    go(T.START, 0, [])
    return out


def _key(counter):
    return tuple(sorted(counter.items()))


def test_composite_features_are_in_the_corpus():
    c = T.composite()
    tr = c.trellis
    # the folded edges of the epsilon part, as stated by hand
    own = {}
    for u, es in tr.edges.items():
        for b, v, p in es:
            if not (str(u).startswith("w_") or str(v).startswith("w_")):
                own.setdefault((u, b, v), []).append(len(p))
    assert {k: sorted(v) for k, v in own.items()} == T.COMPOSITE["edge_params"]
    assert {u: sorted(len(p) for p in ps) for u, ps in tr.ends.items() if ps and not str(u).startswith("w_")} \
        == T.COMPOSITE["end_params"]
    no_end = [u for u in tr.nodes if not tr.ends[u] and u != T.END]
    assert {("E2", "pq", 1), ("M", "rst", 1), ("M", "rst", 2), "w_0_0", T.START} <= set(no_end)
    # ... and the oracle folds the same way: per string the ENUM oracle's paths, as parameter multisets, are
    # the folded trellis' paths (the strings without the wide gadget: a handful of paths each)
    o = T.enum_oracle(c.subset(c.recognized))
    names = o.param_names()
    prow, pcol, pdata, mrow = o.paths()
    kept = [s for s, r in zip(c.strings, c.recognized) if r]
    for i, s in enumerate(kept):
        if b"aa" in s:
            continue
        mine = collections.Counter(_key(p) for p in _fold_paths(tr, s))
        theirs = collections.Counter(
            _key(collections.Counter({names[pcol[q]]: int(pdata[q]) for q in range(prow[l], prow[l + 1])}))
            for l in range(mrow[i], mrow[i + 1]))
        assert mine == theirs, s
    # the features on accepting paths, in strings without the wide gadget and in strings with it: an edge of at
    # least five parameters, a parallel pair, a zero-parameter chain edge, a composite end edge (three or more)
    for with_gadget in (False, True):
        five = pair = chain = xend = three_byte = 0
        for s in kept:
            if (b"aa" in s) != with_gadget:
                continue
            edges, x_edges = T.accepting(tr, s)
            five += any(len(p) >= 5 for *_, p in edges)
            by = collections.Counter((i, u, b, v) for i, u, b, v, _ in edges)
            pair += any(n > 1 and len({p for j, a, bb, d, p in edges if (j, a, bb, d) == k}) == n for k, n in by.items())
            chain += any(len(p) == 0 and isinstance(u, tuple) for _, u, _, _, p in edges)
            three_byte += any(u == ("M", "rst", 2) for _, u, *_ in edges)
            xend += any(len(p) >= 3 for _, p in x_edges)
        assert min(five, pair, chain, xend, three_byte) >= 2, (with_gadget, five, pair, chain, xend, three_byte)
    # the slab route needs the wide gadget before, after and between the features, and at both ends of a string
    gadget = [s for s in kept if b"aa" in s]
    assert any(s.endswith(b"aa") for s in gadget) and any(s.startswith(b"xaax") and len(s) > 4 for s in gadget)
    assert any(not s.startswith(b"xaa") for s in gadget) and any(s.count(b"aa") == 2 for s in gadget)
    assert T.composite_traversal(c).sum() == len(gadget) + 2 and min(len(s) for s in c.strings) == 1
    assert len(np.unique(c.wt)) == len(c.strings) == 22


# -- the reference lies inside the tolerances -------------------------------------------

@pytest.mark.parametrize("seed", T.SEEDS)
def test_trellis_oracle_is_inside_the_gpu_tolerances(seed):
    """log q rtol 1e-11, log-likelihood relative 1e-11, gradient rtol 1e-9
    atol 1e-15 (test_gpu_tier2's): the float64 TRELLIS oracle on the
    composite corpus against long-double sums over the ENUM oracle's paths at
    the same weights"""
    c = T.composite()
    clean = c.subset(c.recognized)
    w, ll, logq, grad = T.trellis_reference(clean, seed)
    o = T.enum_oracle(clean)
    names = o.param_names()
    assert sorted(names) == sorted(w), "a parameter no string uses"
    x = np.array([w[n] for n in names], dtype=LD)
    prow, pcol, pdata, mrow = o.paths()
    path = np.repeat(np.arange(len(prow) - 1), np.diff(prow))
    lw = np.zeros(len(prow) - 1, dtype=LD)
    np.add.at(lw, path, pdata.astype(LD) * x[pcol])
    p = o.p().astype(LD)
    logq_ld, g_ld = np.zeros(len(p), dtype=LD), np.zeros(len(names), dtype=LD)
    post = np.zeros(len(lw), dtype=LD)
    for s in range(len(p)):
        a, b = int(mrow[s]), int(mrow[s + 1])
        e = np.exp(lw[a:b] - lw[a:b].max())
        logq_ld[s] = lw[a:b].max() + np.log(e.sum())
        post[a:b] = p[s] * e / e.sum()
    np.add.at(g_ld, pcol, -pdata.astype(LD) * post[path])
    ll_ld = (p * logq_ld).sum()
    g = np.array([grad[n] for n in names])
    err_q = float(np.max(np.abs(logq - logq_ld) / np.abs(logq_ld)))
    err_g = float(np.max(np.abs(g - g_ld) / np.abs(g_ld)))
    print(f"composite seed {seed}: TRELLIS vs long double over {len(lw)} paths: logq rel {err_q:.2e} "
          f"ll rel {abs(ll - ll_ld) / abs(ll_ld):.2e} grad rel {err_g:.2e}")
    assert np.isfinite(logq).all() and (g < 0).all()
    np.testing.assert_allclose(logq, logq_ld.astype(np.float64), rtol=1e-11)
    assert abs(ll - ll_ld) <= 1e-11 * abs(ll_ld)
    np.testing.assert_allclose(g, g_ld.astype(np.float64), rtol=1e-9, atol=1e-15)


# -- the capacity corpus --------------------------------------------------------------

def test_make_slab_restated():
    assert T.slab_caps(200, 200) == ((452, 683), (4198, 6301))
    for max_len, n_nodes in [(200, 200), (T.CAP_MAX_LEN, 817), (64, 3000), (1000, 100)]:
        for budget in T.TIER0_BUDGETS + (T.TIER1_BUDGET,):
            caps = T.make_slab(budget, max_len, n_nodes)
            if caps is None:
                continue
            cf, ce = caps
            assert cf % 2 == 0 and cf >= 64 and T.slab_total(cf, ce, max_len, n_nodes) <= budget
            # one more frontier entry pair, or 16 more edges, would not fit
            assert T.slab_total(cf + 2, ce + 16, max_len, n_nodes) > budget
    assert T.make_slab(20480, 160, 4500) is None and T.slab_caps(160, 4500)[0] == T.make_slab(40960, 160, 4500)
    assert T.tier_of(452, 683, T.slab_caps(200, 200)) == 0 and T.tier_of(453, 1, T.slab_caps(200, 200)) == 1
    assert T.tier_of(1, 684, T.slab_caps(200, 200)) == 1 and T.tier_of(4199, 1, T.slab_caps(200, 200)) == 2


def test_every_capacity_has_its_three_strings():
    case, fe, caps, boundary = T.capacity()
    tr = case.trellis
    assert caps == T.slab_caps(max(len(s) for s in case.strings), len(tr.nodes)) == ((400, 604), (4146, 6222))
    assert max(len(s) for s in case.strings) == T.CAP_MAX_LEN and len(case.strings) == 18
    # the closed-form counts are the walk's
    for s, (f, e), p in zip(case.strings, fe, case.paths):
        assert T.walk(tr, s) == (f, e, p), s
    case.path_counts()   # (exact as doubles)
    assert sorted(boundary) == [(t, q, d) for t in (0, 1) for q in "ef" for d in (-1, 0, 1)]
    for (tier, which, delta), i in boundary.items():
        f, e = fe[i]
        cf, ce = caps[tier]
        bind, cap, other, other_cap = (f, cf, e, ce) if which == "f" else (e, ce, f, cf)
        assert bind == cap + delta and other <= other_cap - T.CAP_MARGIN, (tier, which, delta, f, e)
        assert T.tier_of(f, e, caps) == tier + (delta == 1)
        assert T.capacity_traversal(case)[i]
    tiers = [T.tier_of(f, e, caps) for f, e in fe]
    # tier 0: five of the plain strings and the four at or under a tier-0 capacity; the c64 visit alone is past
    # tier 0's cap_f; tier 2: the two strings one over a tier-1 capacity
    assert (tiers.count(0), tiers.count(1), tiers.count(2)) == (9, 7, 2)
    assert list(T.capacity_traversal(case)[:6]) == [False, True, True, True, True, False]
