"""Automata for the traversal kernels, built by hand, with their corpora and
the routes that put them on each kernel (test_traversal_gadgets_reference.py,
test_gpu_traversal_gadgets.py) -- test infrastructure, the sibling of
bubble_gadgets.py for the strings that do not compile.

Every automaton is a list of states (name, emissions, transitions), all
weights 0: ^ -> H, H emits x, and behind H the gadgets of bubble_gadgets
(layers, fully connected or k parallel chains, the last layer -> H and $).
fold() restates trellis_model.cpp on such a list (epsilon states folded into
the edges, a chain of nodes per multi-byte emission), walk() runs a string
over the folded trellis as trav_kernel does and counts what it counts.

(a) composite(): an epsilon part behind H (E1: epsilon | z, E2: epsilon | pq,
    M: rst | r) and the 33-node gadget of bubble_gadgets.  The folded trellis
    holds edges of up to six parameters, parallel edges, chain nodes and
    composite end edges; COMPOSITE states them.
(b) db(w1, w2): one two-layer gadget, every state emitting a: D(a) = w1 + w2,
    the quantity build_pull_tables chooses the lanes' item count by.
(c) capacity(): chains of 33, 34 and 64, a (16, 16) layer pair and two unary
    gadgets, and a corpus with strings one under, at and one over each of
    the four slab capacities (make_slab restated in slab_caps)."""
import functools
import math

import numpy as np

from bubble_gadgets import Gadget

START, END = "^", "$"

# -- routes: the environment that sends the traversal strings to each kernel ----

ROUTES = {
    "pull": {"WFSA_TIER2": "1"},                    # wave_pull_kernel
    "push": {"WFSA_TIER2": "1", "WFSA_PULL": "0"},  # wide2_kernel
    "wide": {"WFSA_TIER2": "1", "WFSA_WIDE2": "0"},  # wide_kernel, a block per string
    "slab": {"WFSA_TIER2": "0", "WFSA_WIDE2": "0"},  # trav_kernel on the LDS slabs (wide_kernel past them)
}
ROUTE_KNOBS = ("WFSA_TIER2", "WFSA_PULL", "WFSA_WIDE2")


def set_route(monkeypatch, route):
    for k in ROUTE_KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("WFSA_DENSE", "0")
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)


def confirm_route(route, st, n_strings, n_traversal):
    """stats() says the route was taken; n_traversal: the strings that do not compile"""
    if route == "pull":
        assert st["wave_strings"] > 0 and st["wave_pull"] in (4, 6, 8), st
    elif route == "push":
        assert st["wave_strings"] > 0 and st["wave_pull"] == 0, st
    elif route == "wide":
        assert st["wave_strings"] == 0 and st["tier2_strings"] == n_strings, st
    else:
        assert st["wave_strings"] == 0 and st["fallback_strings"] == n_traversal, st
    if route != "slab":   # WFSA_TIER2=1: the count pass compiles nothing
        assert st["tier2_strings"] == n_strings and st["compiled_strings"] == 0, st


# -- automata ------------------------------------------------------------------

def gadget_states(g):
    """the states of one bubble_gadgets.Gadget (every state emits its letters)"""
    out, k = [], len(g.widths)
    for i, w in enumerate(g.widths):
        for j in range(w):
            nxt = [g.state(i + 1, m) for m in (range(g.widths[i + 1]) if g.full else [j])] if i + 1 < k else ["H", END]
            out.append((g.state(i, j), list(g.letters), nxt))
    return out


def automaton(gadgets, h_extra=(), extra=()):
    """^ -> H; H emits x and goes to every gadget's first layer, $ and h_extra"""
    first = [g.state(0, j) for g in gadgets for j in range(g.widths[0])]
    states = [(START, [""], ["H"]), ("H", ["x"], first + [END] + list(h_extra))] + list(extra)
    for g in gadgets:
        states += gadget_states(g)
    assert len({n for n, _, _ in states}) == len(states)
    return states


def wfsa_text(states):
    t = ["", START, END]
    for name, em, tr in states:
        t += [name + " " + " ".join(f"{e} 0" for e in em), name + " " + " ".join(f"{d} 0" for d in tr)]
    return "\n".join(t) + "\n"


def param_names(states):
    """(state, kind, label) of every parameter: a state's emissions and its
    transitions are parameters where it has more than one of them"""
    out = []
    for name, em, tr in states:
        out += [(name, "E", e) for e in em if len(em) > 1] + [(name, "T", d) for d in tr if len(tr) > 1]
    return out


class Trellis:
    """fold()'s result: edges[u] = [(byte, v, parameters)], ends[u] = [parameters]"""

    def __init__(self, nodes, edges, ends):
        self.nodes, self.edges, self.ends = nodes, edges, ends

    @property
    def n_edges(self):
        return sum(len(v) for v in self.edges.values())

    @property
    def n_end_edges(self):
        return sum(len(v) for v in self.ends.values())

    @property
    def n_entries(self):
        return sum(len(p) for v in self.edges.values() for _, _, p in v) + sum(len(p) for v in self.ends.values() for p in v)

    def dests(self, byte):
        """D(byte): the nodes an edge of that byte enters"""
        return {v for es in self.edges.values() for b, v, _ in es if b == byte}

    def byte_edges(self, byte):
        return sum(b == byte for es in self.edges.values() for b, _, _ in es)


def fold(states):
    """trellis_model.cpp restated: from every state S a walk over the
    transitions; a target's epsilon emission goes on from the target with the
    parameters met so far, any other emission closes an edge of S on its
    first byte -- into the target, or into the first of the emission's chain
    nodes (T, emission, k), whose own edges carry no parameter; a transition
    into $ closes an end edge of S.  The nodes are the states, $ and the chain
    nodes"""
    em = {n: e for n, e, _ in states}
    tr = {n: t for n, _, t in states}
    nodes = [n for n, _, _ in states] + [END]
    edges = {n: [] for n in nodes}
    ends = {n: [] for n in nodes}

    def expand(S, X, cur, on_path):
        for T in tr[X]:
            tp = [(X, "T", T)] if len(tr[X]) > 1 else []
            if T == END:
                ends[S].append(tuple(cur + tp))
                continue
            for e in em[T]:
                ep = [(T, "E", e)] if len(em[T]) > 1 else []
                if e == "":
                    assert T not in on_path, "epsilon cycle"
                    expand(S, T, cur + tp + ep, on_path | {T})
                else:
                    edges[S].append((e[0], T if len(e) == 1 else (T, e, 1), tuple(cur + tp + ep)))

    for S, _, _ in states:
        expand(S, S, [], {S})
    for T, es, _ in states:
        for e in es:
            for k in range(1, len(e)):
                nodes.append((T, e, k))
                edges[(T, e, k)] = [(e[k], (T, e, k + 1) if k + 1 < len(e) else T, ())]
                ends[(T, e, k)] = []
    return Trellis(nodes, edges, ends)


def walk(tr, s):
    """string s (bytes) over the folded trellis, as trav_kernel's forward:
    (frontier entries F, live edges E, accepting paths).  The start entry
    counts as 1, every distinct node of a position once, every edge taken
    once; a frontier that dies ends the walk"""
    front, F, E = {START: 1}, 1, 0
    for c in s.decode("latin-1"):
        nxt = {}
        for u, n in front.items():
            for b, v, _ in tr.edges[u]:
                if b == c:
                    E += 1
                    nxt[v] = nxt.get(v, 0) + n
        F += len(nxt)
        front = nxt
        if not front:
            break
    return F, E, sum(n * len(tr.ends[u]) for u, n in front.items())


def accepting(tr, s):
    """the edges (position, u, byte, v, parameters) and end edges (u,
    parameters) that lie on an accepting path of s"""
    text = s.decode("latin-1")
    fw = [{START}]
    for c in text:
        fw.append({v for u in fw[-1] for b, v, _ in tr.edges[u] if b == c})
    live = {u for u in fw[-1] if tr.ends[u]}
    x_edges = [(u, p) for u in sorted(live, key=str) for p in tr.ends[u]]
    out = []
    for i in range(len(text) - 1, -1, -1):
        here = [(i, u, b, v, p) for u in fw[i] for b, v, p in tr.edges[u] if b == text[i] and v in live]
        out += here
        live = {u for _, u, *_ in here}
    return out, x_edges


class Case:
    """an automaton and its corpus: the text, the packed strings, pairwise
    distinct weights 1 + sqrt(i + 2) and the hand-stated path counts"""

    def __init__(self, states, strings, paths):
        assert len(set(strings)) == len(strings) == len(paths), "a string twice"
        self.states, self.strings, self.paths = states, list(strings), np.array(paths, dtype=object)
        self.text = wfsa_text(states)
        self.sym = np.frombuffer(b"".join(self.strings), dtype=np.uint8).copy()
        self.off = np.concatenate([[0], np.cumsum([len(s) for s in self.strings])]).astype(np.int64)
        self.wt = 1.0 + np.sqrt(np.arange(len(self.strings)) + 2.0)
        assert len(np.unique(self.wt)) == len(self.wt)

    @functools.cached_property
    def trellis(self):
        return fold(self.states)

    @property
    def recognized(self):
        return np.array([p > 0 for p in self.paths])

    def path_counts(self):
        """as doubles; every count is exactly representable"""
        assert all(int(float(p)) == p for p in self.paths)
        return np.array([float(p) for p in self.paths])

    def subset(self, mask):
        """the strings where mask holds, each with the weight it has here"""
        keep = np.flatnonzero(np.asarray(mask, dtype=bool))
        c = Case(self.states, [self.strings[i] for i in keep], [self.paths[i] for i in keep])
        c.wt = self.wt[keep]
        return c


# -- (a) the composite automaton -------------------------------------------------

WIDE = Gadget("w", "a", (16, 15))   # 33 nodes: beyond the compile limits (bubble_gadgets t1615)
WIDE_PATHS = 16 * 15

# the epsilon part: the states behind H
EPS_PART = [("E1", ["", "z"], ["E2", "M"]),
            ("E2", ["", "pq"], ["M", END]),
            ("M", ["rst", "r"], ["H", END, "E2"])]

# What folding makes of it, stated by hand; test_traversal_gadgets_reference.py
# checks each line against fold() and against the oracle's path matrices.
#   edges of H on r into M: over E1 E2 (6 parameters) and over E1 (4): a parallel pair;
#   the same pair on r into the first chain node of rst; on p (E1, E2: 4) into pq's chain node
#   end edges of H: its own $ (1 parameter) and over E1 E2 (5)
#   end edges of M: its own $ (1) and over E2 (3); of E1: over E2 (3); of E2: its own (1)
#   chain nodes: one of pq, two of rst; zero-parameter edges q, s, t; no end edge
COMPOSITE = dict(
    edge_params={("H", "r", "M"): [4, 6], ("H", "r", ("M", "rst", 1)): [4, 6], ("H", "p", ("E2", "pq", 1)): [4],
                 ("H", "z", "E1"): [2], ("E1", "r", "M"): [2, 4], ("E1", "r", ("M", "rst", 1)): [2, 4],
                 ("E1", "p", ("E2", "pq", 1)): [2], ("E2", "r", "M"): [2], ("E2", "r", ("M", "rst", 1)): [2],
                 ("M", "x", "H"): [1], ("M", "r", "M"): [4], ("M", "r", ("M", "rst", 1)): [4],
                 ("M", "p", ("E2", "pq", 1)): [2],
                 (START, "x", "H"): [0], (("E2", "pq", 1), "q", "E2"): [0], (("M", "rst", 1), "s", ("M", "rst", 2)): [0],
                 (("M", "rst", 2), "t", "M"): [0]},
    end_params={"H": [1, 5], "M": [1, 3], "E1": [3], "E2": [1]},
)

# (string, accepting paths): the ways are products of
#   H -r|rst-> M 2, H -z-> E1 1, H -pq-> E2 1, H -aa-> 240 (then x -> H 1), E1 -r|rst-> M 2, E1 -pq-> E2 1,
#   E2 -r|rst-> M 1, M -x-> H 1, M -r|rst-> M 1, M -pq-> E2 1; ends: H 2, M 2, E1 1, E2 1, the gadget's last layer 1
COMPOSITE_STRINGS = [
    (b"x", 2),                 # length 1: H's two end edges
    (b"xr", 2 * 2),            # the parallel pair, M's composite end edge
    (b"xrst", 2 * 2),          # the pair into the chain of rst
    (b"xz", 1),                # E1: its only end edge is composite
    (b"xzr", 2 * 2),
    (b"xpq", 1),               # a four-parameter edge into the chain of pq
    (b"xzpq", 1),
    (b"xpqr", 2),
    (b"xrx", 2 * 2),
    (b"xrr", 2 * 2),           # M -> E2 -> M
    (b"xrstpqrst", 2 * 2),
    (b"xzrstx", 2 * 2),
    # with the wide gadget: the whole string runs on the traversal path
    (b"xaa", 240),
    (b"xaax", 240 * 2),                    # H's composite end edge behind the gadget
    (b"xaaxr", 240 * 2 * 2),               # the pair behind it, at the string's end
    (b"xrxaa", 2 * 240),                   # and before it
    (b"xaaxpq", 240),
    (b"xzrstxaax", 2 * 240 * 2),
    (b"xaaxrstxaa", 240 * 2 * 240),        # mid-string, between two visits
    (b"xpqrxaaxz", 240),
    # rejected: a byte no state emits, in mid-string; one a too many for the gadget
    (b"xaakx", 0),
    (b"xaaa", 0),
]


@functools.lru_cache(maxsize=None)
def composite():
    states = automaton([WIDE], h_extra=["E1"], extra=EPS_PART)
    return Case(states, [s for s, _ in COMPOSITE_STRINGS], [n for _, n in COMPOSITE_STRINGS])


def composite_traversal(c):
    """per string: it does not compile (it visits the wide gadget)"""
    return np.array([b"aa" in s for s in c.strings])


# -- (b) the D(b) family ----------------------------------------------------------

UNARY = Gadget("u1", "u", (1,))
# total width -> wave_pull: build_pull_tables takes 4 items per lane up to 256
# destinations, 6 up to 384, 8 up to 512 and builds no pull layout beyond.
# At 64 NI destinations deal() fills every lane to exactly NI items; one
# destination more cannot be held with NI per lane and takes the next step
DB_WIDTHS = {256: 4, 257: 6, 384: 6, 385: 8, 512: 8, 513: 0}
DB_FIRST = 8
# (40, 472): D = 512 and 19,868 parameters.  pull_lds: the gradient table of
# (n_params + 64) doubles beside four waves' rows of 512 doubles is
# 159,456 + 16,384 bytes > 162,816, so the waves add into the global
# fixed-point accumulators; at (8, 504) the table takes 40,928 bytes
DB_GLOBAL = (40, 472)


@functools.lru_cache(maxsize=None)
def db(w1, w2):
    """the visit mid-string, at the string's end, behind a second visit and
    behind a unary visit, and three strings without it"""
    g = Gadget("g", "a", (w1, w2))
    p = w1 * w2
    strings = [(b"xaax", p), (b"xaa", p), (b"xaaxaa", p * p), (b"xuxaax", p), (b"x", 1), (b"xux", 1), (b"xu", 1)]
    return Case(automaton([g, UNARY]), [s for s, _ in strings], [n for _, n in strings])


def db_n_params(w1, w2):
    """H: w1 + 1 (u1) + 1 ($); first layer: w2 each; second layer and u1: H and $"""
    return w1 + 2 + w1 * w2 + 2 * w2 + 2


# -- (c) the capacity family ------------------------------------------------------

CAP_GADGETS = {g.name: g for g in [
    Gadget("u1", "u", (1,)), Gadget("v1", "v", (1,)),
    Gadget("c33", "b", (33,) * 4, full=False), Gadget("c34", "c", (34,) * 4, full=False),
    Gadget("c64", "d", (64,) * 8, full=False),
    Gadget("f1616", "g", (16, 16)),
]}
CAP_MAX_LEN = 160          # a unary string of this length fixes max_len, which the capacities depend on
CAP_MARGIN = 48            # the quantity that does not bind stays this far under its capacity
TIER0_BUDGETS = (20480, 40960)
TIER1_BUDGET = 163840 - 1024   # kLdsPerCu - 1024


def slab_total(cap_f, cap_e, max_len, n_nodes):
    """slab_layout's total: alpha, beta (8 each) and the node (4) per frontier
    entry, three ints per live edge, three ints per position, the slot map"""
    return (20 * cap_f + 12 * cap_e + 12 * (max_len + 2) + 4 * n_nodes + 15) & ~15


def make_slab(budget, max_len, n_nodes):
    """wfsa_dev.hip make_slab restated: (cap_f, cap_e), or None"""
    rem = budget - (12 * (max_len + 2) + 4 * n_nodes + 16)
    if rem < 38 * 64:
        return None
    cap_f = (rem // 38) & ~1
    cap_e = (rem - 20 * cap_f) // 12
    while slab_total(cap_f, cap_e, max_len, n_nodes) > budget and cap_e > 64:
        cap_e -= 16
    return None if slab_total(cap_f, cap_e, max_len, n_nodes) > budget else (cap_f, cap_e)


def slab_caps(max_len, n_nodes):
    """((cap_f, cap_e) of tier 0, of tier 1), as configure_tiers finds them"""
    t0 = next((c for c in (make_slab(b, max_len, n_nodes) for b in TIER0_BUDGETS) if c), None)
    t1 = make_slab(TIER1_BUDGET, max_len, n_nodes)
    return (t0 or t1), t1


def tier_of(F, E, caps):
    """the tier trav_kernel's check leaves a string on: it overflows a slab
    when F > cap_f or E > cap_e"""
    for t, (cf, ce) in enumerate(caps):
        if F <= cf and E <= ce:
            return t
    return 2


def visit_counts(g, end):
    """(frontier entries, live edges, bytes) one visit adds: its layers and H
    again behind it -- at the string's end neither H nor the edges back to it"""
    w = g.widths
    inner = sum(w[i] * w[i + 1] if g.full else w[i] for i in range(len(w) - 1))
    return (sum(w), w[0] + inner, len(w)) if end else (sum(w) + 1, w[0] + inner + w[-1], len(w) + 1)


def cap_string(visits, end):
    """x V x V ... x (end: without the last x), each visit its gadget's letter once per layer"""
    s = "x" + "x".join(CAP_GADGETS[n].letters * len(CAP_GADGETS[n].widths) for n in visits)
    return (s if end or not visits else s + "x").encode()


def cap_counts(visits, end):
    """(F, E, paths) of cap_string(visits, end) in closed form: start and H, then the visits"""
    F, E = 2, 1
    for k, n in enumerate(visits):
        f, e, _ = visit_counts(CAP_GADGETS[n], end and k + 1 == len(visits))
        F, E = F + f, E + e
    return F, E, math.prod(CAP_GADGETS[n].paths for n in visits)


def _solve(target, bind, other_cap, use):
    """the shortest string whose binding quantity (0: F, 1: E) is exactly
    target and whose other quantity stays CAP_MARGIN under other_cap: counts
    of the gadgets in `use`, the last of them at the string's end or not,
    filled with unary visits (2 entries and 2 edges each) in front"""
    best = None
    mid = [visit_counts(CAP_GADGETS[n], False) for n in use]
    for counts in np.ndindex(*[2 + target // m[bind] for m in mid]):
        if not any(counts):
            continue
        q = [(2, 1, 1)[k] + sum(c * m[k] for c, m in zip(counts, mid)) for k in range(3)]
        last = max(i for i, c in enumerate(counts) if c)
        at_end = visit_counts(CAP_GADGETS[use[last]], True)
        for end in (False, True):
            if end:
                q = [a - m + e for a, m, e in zip(q, mid[last], at_end)]
            rest = target - q[bind]
            if rest < 0 or rest % 2 or q[1 - bind] + rest > other_cap - CAP_MARGIN or q[2] + rest >= CAP_MAX_LEN:
                continue
            if best is None or q[2] + rest < best[0]:
                best = (q[2] + rest, counts, end, rest // 2)
    assert best is not None, (target, bind)
    _, counts, end, n_unary = best
    visits = ["u1", "v1"] * (n_unary // 2) + ["u1"] * (n_unary % 2) + [n for n, k in zip(use, counts) for _ in range(k)]
    assert cap_counts(visits, end)[bind] == target and len(cap_string(visits, end)) == best[0]
    return visits, end


@functools.lru_cache(maxsize=None)
def capacity():
    """(the case, per string (F, E), the capacities, the boundary strings:
    (tier, 'f' | 'e', -1 | 0 | 1) -> string index).  The chains bind cap_f
    (F ~ E), the (16, 16) pair binds cap_e (E ~ 8.7 F); the unary string of
    CAP_MAX_LEN bytes is the longest, so the capacities the corpus is built
    to are the ones the device computes from it"""
    states = automaton(list(CAP_GADGETS.values()))
    n_nodes = len(fold(states).nodes)
    caps = slab_caps(CAP_MAX_LEN, n_nodes)
    specs = [([], False), (["c33"], False), (["c34"], True), (["f1616"], False), (["c64"], True),
             (["u1", "v1"] * (CAP_MAX_LEN // 4), True)]
    assert len(cap_string(*specs[-1])) == CAP_MAX_LEN
    boundary = {}
    for tier, (cf, ce) in enumerate(caps):
        for which, cap, other, use in (("f", cf, ce, ["c33", "c34", "c64"]), ("e", ce, cf, ["f1616", "c33", "c34"])):
            for delta in (-1, 0, 1):
                boundary[(tier, which, delta)] = len(specs)
                specs.append(_solve(cap + delta, 0 if which == "f" else 1, other, use))
    strings = [cap_string(v, e) for v, e in specs]
    counts = [cap_counts(v, e) for v, e in specs]
    case = Case(states, strings, [p for _, _, p in counts])
    assert max(len(s) for s in strings) == CAP_MAX_LEN
    return case, [(f, e) for f, e, _ in counts], caps, boundary


def capacity_traversal(case):
    """per string: it visits a gadget beyond the compile limits (all but the unary ones are)"""
    return np.array([any(c in s for c in b"bcdg") for s in case.strings])


# -- the reference ----------------------------------------------------------------

SEEDS = (11, 12)


def weights(names, seed):
    """rng.normal(-1.2, 0.6) per parameter, by name"""
    keys = sorted(names)
    return dict(zip(keys, np.random.default_rng(seed).normal(-1.2, 0.6, size=len(keys))))


def trellis_reference(case, seed):
    """the TRELLIS oracle at weights(seed): (weights by name, log-likelihood,
    log q per string, gradient by name).  The corpus must hold recognized
    strings only: the oracle and the device then normalise p over the same
    strings"""
    from oracle import Oracle, TRELLIS
    o = Oracle.from_arrays(case.text, case.sym, case.off, case.wt, mode=TRELLIS)
    names = o.full_param_names()
    w = weights(names, seed)
    ll, logq, grad = o.trellis_eval(np.array([w[n] for n in names]))
    logq.setflags(write=False)
    return w, ll, logq, dict(zip(names, grad))


def enum_oracle(case, max_paths=10_000_000):
    from oracle import ENUM, Oracle
    return Oracle.from_arrays(case.text, case.sym, case.off, case.wt, mode=ENUM, max_paths=max_paths)
