"""The hand-built bubble cases (bubble_gadgets.py) checked without a device:
the counts the GPU tests compute from the visits, and the ENUM oracle they
compare with against a long-double log-sum-exp over the enumerated paths, at
the GPU tests' own tolerances -- so the reference is known to lie inside them
(test_gpu_bubble_classes.py)."""
import functools

import numpy as np
import pytest

import bubble_gadgets as B

LD = np.longdouble
CASES = ["all", "big", "big1", "limits", "limits_14k", "mixed", "mixed_m2", 3, 129]

# (nodes, edges, paths) of every gadget's bubble, stated by hand
COUNTS = {
    "d2": (4, 4, 2), "d2b": (4, 4, 2), "t3": (5, 6, 3), "c22": (6, 6, 2), "q4": (6, 8, 4), "c222": (8, 8, 2),
    "f22": (6, 8, 4), "c33": (8, 9, 3), "s6": (8, 12, 6), "c2222": (10, 10, 2), "s7": (9, 14, 7), "m2": (4, 4, 2),
    "l1515": (32, 255, 225), "l1416": (32, 254, 224), "l101010": (32, 220, 1000), "t1615": (33, 271, 240),
    "u1": (3, 2, 1), "v1": (3, 2, 1),
}


def test_every_gadget_lands_in_its_stated_class():
    assert set(COUNTS) == set(B.GADGETS)
    for name, g in B.GADGETS.items():
        assert (g.nodes, g.edges, g.paths) == COUNTS[name], name
        if g.klass is None:   # a unary gadget: every position a cut node, no bubble
            assert g.widths == (1,)
            continue
        assert B.rule_class(g.nodes, g.edges, g.multi) == g.klass, name
        assert g.shape == 0 or g.klass in ("A", "B")
    # one step past each bound of the small classes, and the multi-parameter diamond
    assert B.rule_class(4, 4, False) == "A" and B.rule_class(5, 4, False) == "B" and B.rule_class(4, 5, False) == "B"
    assert B.rule_class(8, 8, False) == "B" and B.rule_class(8, 9, False) == "big" and B.rule_class(9, 8, False) == "big"
    assert B.rule_class(4, 4, True) == "big"
    assert B.rule_class(32, 255, False) == "big" and B.rule_class(33, 255, False) == "trav"
    assert B.rule_class(32, 256, False) == "trav"


def _layered_edges(w):
    return w[0] + sum(a * b for a, b in zip(w, w[1:])) + w[-1]


def _splits(total):
    """every sequence of positive layer widths with the given sum"""
    if total == 0:
        yield ()
    for first in range(1, total + 1):
        for rest in _splits(total - first):
            yield (first,) + rest


def test_255_edges_is_the_most_a_region_of_32_nodes_can_have():
    """A region is layered by position: a node of layer i has edges to layer
    i + 1 only, so w1 + sum w_i w_{i+1} + wk bounds its edges.  Over every
    split of at most 30 inner nodes the bound's maximum is 255, reached by
    (15, 15) alone: best[t][l] is the most edges before the closing ones of a
    split of t nodes whose last layer has l, ways[t][l] the splits reaching it"""
    inner = B.MAX_NODES - 2
    best = [[-1] * (inner + 1) for _ in range(inner + 1)]
    ways = [[0] * (inner + 1) for _ in range(inner + 1)]
    for t in range(1, inner + 1):
        for l in range(1, t + 1):
            cand = [(l, 1)] if l == t else []
            cand += [(best[t - l][p] + p * l, ways[t - l][p]) for p in range(1, t - l + 1)]
            best[t][l] = max(c for c, _ in cand)
            ways[t][l] = sum(n for c, n in cand if c == best[t][l])
    closed = [(best[t][l] + l, ways[t][l], t, l) for t in range(1, inner + 1) for l in range(1, t + 1)]
    top = max(c for c, *_ in closed)
    assert top == B.MAX_EDGES == 255
    assert [(n, t, l) for c, n, t, l in closed if c == top] == [(1, 30, 15)]
    assert _layered_edges((15, 15)) == 255 and _layered_edges((14, 16)) == 254 and _layered_edges((10, 10, 10)) == 220
    assert 2 + 16 + 15 == 33 > B.MAX_NODES   # (16, 15): past the node limit
    # the recurrence against every split written out, for the sizes where that is quick
    for t in range(1, 13):
        by_last = {}
        for w in _splits(t):
            by_last.setdefault(w[-1], []).append(_layered_edges(w) - w[-1])
        for l, vals in by_last.items():
            assert best[t][l] == max(vals) and ways[t][l] == vals.count(max(vals)), (t, l)
    # the staging rounds of 255 edges on 64 lanes: four, the last with 63 lanes; 254: an even
    # count without a spare entry; big_lds_edges = (edges + 1) & ~1
    assert -(-255 // 64) == 4 and 255 - 3 * 64 == 63
    assert (255 + 1) & ~1 == 256 and (254 + 1) & ~1 == 254


@functools.lru_cache(maxsize=None)
def _oracle(key):
    return B.oracle(key)


@pytest.mark.parametrize("key", CASES, ids=str)
def test_path_counts_are_the_products_of_the_visits(key):
    c = B.get(key)
    pc = _oracle(key).path_counts()
    assert np.array_equal(pc, c.path_counts())
    assert (pc > 0).all()   # every string is recognized
    e = c.expected()
    print(f"{key}: {len(c.strings)} strings, {int(pc.sum())} paths, expected {e}")
    assert e["small_bubbles_a"] + e["small_bubbles_b"] + e["big_bubbles"] == sum(len(b) for b in c.bubbles())


def test_the_corpora_hold_what_the_gpu_tests_need():
    a = B.case("all")
    e = a.expected()
    assert e["max_bubble_nodes"] == 32 and e["max_bubble_edges"] == 255 and e["fallback_strings"] == 3
    assert e["small_bubbles_a"] > 0 and e["small_bubbles_b"] > e["shaped_bubbles"] - e["small_bubbles_a"] > 0
    # every bubble gadget mid-string and at the end of a string
    for name, g in B.GADGETS.items():
        if g.klass in ("A", "B", "big") and name != "d2b":
            assert any(vs == [name] and s.endswith(b"x") for vs, s in zip(a.visits, a.strings)), name
            assert any(vs == [name] and not s.endswith(b"x") for vs, s in zip(a.visits, a.strings)), name
    assert all(g.klass == "big" for bs in B.case("big").bubbles() for g in bs)
    assert {g.name for bs in B.case("limits").bubbles() for g in bs} == set(B.LIMITS)
    # mixed: strings of one, two and three bubbles; A+B, A+big, B+big and A+B+big
    for key in ("mixed", "mixed_m2"):
        kinds = {tuple(sorted(g.klass for g in bs)) for bs in B.case(key).bubbles()}
        assert {("A", "B"), ("A", "big"), ("B", "big"), ("A", "B", "big")} <= kinds
        assert {len(k) for k in kinds} == {1, 2, 3}
    # the two-emission diamond switches the delta format off: the corpora without it hold no two-letter state
    multi = {key: any(B.GADGETS[n].multi for n in B.get(key).names) for key in CASES}
    assert multi == {"all": True, "big": True, "big1": False, "limits": False, "limits_14k": False, "mixed": False, "mixed_m2": True,
                     3: False, 129: False}
    for n in (1, 2, 3, 63, 64, 65, 129):
        c = B.lanes(n)
        flat = [g.name for bs in c.bubbles() for g in bs]
        assert sum(vs[-1] == "d2b" and s.endswith(b"x") for vs, s in zip(c.visits, c.strings)) == n
        assert sum(vs[-1] == "c22" and s.endswith(b"x") for vs, s in zip(c.visits, c.strings)) == n
        assert flat.count("t3") == 3 and flat.count("d2") == 3


def _long_double(o, x):
    """(log q per string, KL, gradient) from the enumerated paths in long double"""
    from oracle.hessian import HessianOracle
    h = HessianOracle(o)
    mrow, p = np.asarray(h.mrow), h.p.astype(LD)
    P = h.P.astype(LD)
    lw = P @ np.asarray(x, dtype=LD)
    logq = np.zeros(len(p), dtype=LD)
    post = np.zeros(len(lw), dtype=LD)
    for s in range(len(p)):
        a, b = int(mrow[s]), int(mrow[s + 1])
        m = lw[a:b].max()
        e = np.exp(lw[a:b] - m)
        logq[s] = m + np.log(e.sum())
        post[a:b] = p[s] * e / e.sum()
    kl = (p * np.log(p)).sum() - (p * logq).sum()
    return logq, kl, -(P.T @ post)


@pytest.mark.parametrize("seed", B.SEEDS)
@pytest.mark.parametrize("key", CASES, ids=str)
def test_enum_oracle_is_inside_the_gpu_tolerances(key, seed):
    """log q rtol 1e-12 atol 1e-12, KL rel 1e-11, gradient rtol 1e-10 atol
    1e-15 (test_gpu_regimes._check_evaluation's): the float64 oracle against
    the long-double sums at the same weights"""
    o, names, _ = B.perturbed_oracle(key, seed)
    kl, _ = o.objective_grad()
    logq_ld, kl_ld, grad_ld = _long_double(o, o.x())
    logq, grad = o.logq(), o.grad()
    err_q = float(np.max(np.abs(logq - logq_ld) / np.maximum(np.abs(logq_ld), 1e-300)))
    err_g = float(np.max(np.abs(grad - grad_ld) / np.maximum(np.abs(grad_ld), 1e-300)))
    print(f"{key} seed {seed}: oracle vs long double: logq rel {err_q:.2e} KL rel {abs(kl - kl_ld) / abs(kl_ld):.2e} "
          f"grad rel {err_g:.2e}")
    assert np.isfinite(logq).all() and np.isfinite(grad).all()
    np.testing.assert_allclose(logq, logq_ld.astype(np.float64), rtol=1e-12, atol=1e-12)
    assert abs(kl - kl_ld) <= 1e-11 * abs(kl_ld)
    np.testing.assert_allclose(grad, grad_ld.astype(np.float64), rtol=1e-10, atol=1e-15)
    # and the copy the GPU tests share is this evaluation
    _, kl_r, grad_r, logq_r = B.reference(key, seed)
    assert kl_r == kl and np.array_equal(logq_r, logq)
    assert np.array_equal(grad_r, [dict(zip(names, grad))[n] for n in sorted(names)])
