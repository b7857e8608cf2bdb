"""Automata whose bubbles are chosen by hand, and the corpora the bubble-class
tests share (test_bubble_gadgets_reference.py, test_gpu_bubble_classes.py) --
test infrastructure, in the style of hf_reference.ladder_text.

    ^ -> H;  H emits x;  H -> the first layer of every gadget, and $
    a gadget: layers of widths (w1 .. wk), fully connected layer to layer or
    k parallel chains (state j of a layer -> state j of the next); the last
    layer -> H and $; every state of a gadget emits the gadget's own letter

H is the only state that emits x, so it is a cut node wherever it occurs, and
a string  x aa x bbb x  holds one bubble per gadget visit: H, the layers and H
again (2 + sum w nodes; w1 + the inner edges + wk edges).  A visit that ends
the string has the same counts: the cut node is the virtual end node and the
last layer's end edges take the place of its edges back to H.  Every state
has one emission, so no emission is a parameter; a transition is a parameter
unless it is its state's only one (the inner edges of chains carry none).

The unary gadgets (one state each, letters u and v) make no bubble: sequences
of them give many distinct strings around the same bubbles.  One gadget has
two letters per state, the two-emission diamond: its entering edges carry a
transition and an emission parameter each (a multi-parameter edge: a big
bubble whatever its size).  A model with such an edge keeps the 16-bit streams
(no delta format, so no QN update inside the stream kernel), which is why the
unary letters are two one-letter states and not one state with two, and why
only some corpora hold that diamond.

The class of a bubble, as the device's preparation decides it
(w-fsa_amd/csrc/wfsa_dev.hip, the classification loop; fb_kernels.hip
compile_walk for the limits):

    more than 32 nodes or 255 edges           the string leaves the compiled path
    <= 4 nodes, <= 4 edges, one-parameter     class A
    <= 8 nodes, <= 8 edges, one-parameter     class B
    otherwise                                 big

Each gadget below states its class (and, for a small one, the structure id of
fb_kernels.hpp's lists) by hand; test_bubble_gadgets_reference.py checks the
statements against the rule and the counts."""
import functools
import math

import numpy as np

MAX_NODES, MAX_EDGES = 32, 255   # compile_walk's limits


class Gadget:
    def __init__(self, name, letters, widths, full=True, klass=None, shape=0):
        assert full or len(set(widths)) == 1, "chains keep their width"
        self.name, self.letters, self.widths, self.full = name, letters, tuple(widths), full
        self.klass, self.shape = klass, shape   # "A", "B", "big", "trav"; None: no bubble (a unary gadget)

    @property
    def multi(self):
        """an edge into one of its states carries two parameters"""
        return len(self.letters) > 1

    @property
    def nodes(self):
        return 2 + sum(self.widths)

    @property
    def edges(self):
        w = self.widths
        inner = sum(w[i] * w[i + 1] if self.full else w[i] for i in range(len(w) - 1))
        return w[0] + inner + w[-1]

    @property
    def paths(self):
        return math.prod(self.widths) if self.full else self.widths[0]

    def state(self, layer, j):
        return f"{self.name}_{layer}_{j}"


GADGETS = {g.name: g for g in [
    # the unary gadgets: no bubble, two letters between them
    Gadget("u1", "u", (1,)),
    Gadget("v1", "v", (1,)),
    # class A: the diamond (a second one with parameters of its own for the lane-group corpora)
    Gadget("d2", "a", (2,), klass="A", shape=1),
    Gadget("d2b", "q", (2,), klass="A", shape=1),
    # class B, listed structures
    Gadget("t3", "b", (3,), klass="B", shape=2),
    Gadget("c22", "c", (2, 2), full=False, klass="B", shape=1),
    Gadget("q4", "d", (4,), klass="B", shape=5),
    Gadget("c222", "e", (2, 2, 2), full=False, klass="B", shape=3),
    # class B, a structure without compiled-in sweeps
    Gadget("f22", "f", (2, 2), klass="B", shape=0),
    # big, every edge with at most one parameter: one past each class-B bound
    Gadget("c33", "g", (3, 3), full=False, klass="big"),          # 8 nodes, 9 edges
    Gadget("s6", "h", (6,), klass="big"),                         # 8 nodes, 12 edges
    Gadget("c2222", "i", (2, 2, 2, 2), full=False, klass="big"),  # 10 nodes, 10 edges
    Gadget("s7", "j", (7,), klass="big"),                         # 9 nodes, 14 edges
    # big only because of its two-parameter edges: the diamond with two emissions per state
    Gadget("m2", "kl", (2,), klass="big"),
    # the compile limits
    Gadget("l1515", "m", (15, 15), klass="big"),                  # 32 nodes, 255 edges: both limits
    Gadget("l1416", "n", (14, 16), klass="big"),                  # 32 nodes, 254 edges
    Gadget("l101010", "o", (10, 10, 10), klass="big"),            # 32 nodes, 220 edges
    Gadget("t1615", "p", (16, 15), klass="trav"),                 # 33 nodes: traversal
]}
SMALL = ["d2", "t3", "c22", "q4", "c222", "f22"]
BIG = ["c33", "s6", "c2222", "s7", "m2"]
LIMITS = ["l1515", "l1416", "l101010"]


# The limit corpus with the parameter count raised.  A stream-kernel block of
# 1024 threads stages 8 bytes per parameter and, fused, 16 waves' big-bubble
# staging of big_stage_bytes(256) = 3,584 bytes each in 162,816 bytes of LDS:
# the bubbles fit beside the table up to about 13,180 parameters; past 20,303
# the table itself is not staged (tests/test_gpu_regimes.py)
LIMITS_PAD = {"limits_12k": 5_860, "limits_14k": 6_610, "limits_23k": 11_110}


def rule_class(nodes, edges, multi):
    """the classification rule restated (the module docstring's table)"""
    if nodes > MAX_NODES or edges > MAX_EDGES:
        return "trav"
    if multi:
        return "big"
    return "A" if nodes <= 4 and edges <= 4 else "B" if nodes <= 8 and edges <= 8 else "big"


def wfsa_text(names, pad=0):
    """the automaton over the named gadgets, every weight 0.  pad: a chain of
    that many more states behind H that emit y, two transitions each -- no
    string of the corpora holds a y, so their 2 pad + 1 parameters are never
    used (the learners trim them) and only raise the automaton's parameter
    count, by which the device chooses its regime"""
    gs = [GADGETS[n] for n in names]
    assert len({c for g in gs for c in g.letters} | {"x", "y"}) == 2 + sum(len(g.letters) for g in gs)
    t = ["", "^", "$", "^  0", "^ H 0", "H x 0",
         "H " + " ".join(f"{g.state(0, j)} 0" for g in gs for j in range(g.widths[0])) + " pad_0 0" * (pad > 0) + " $ 0"]
    for i in range(pad):
        t += [f"pad_{i} y 0", f"pad_{i} " + (f"pad_{i + 1}" if i + 1 < pad else "H") + " 0 $ 0"]
    for g in gs:
        k = len(g.widths)
        for i, w in enumerate(g.widths):
            for j in range(w):
                t.append(g.state(i, j) + " " + " ".join(f"{c} 0" for c in g.letters))
                if i + 1 < k:
                    nxt = range(g.widths[i + 1]) if g.full else [j]
                    t.append(g.state(i, j) + " " + " ".join(f"{g.state(i + 1, m)} 0" for m in nxt))
                else:
                    t.append(g.state(i, j) + " H 0 $ 0")
    return "\n".join(t) + "\n"


def visit(name, letters=None):
    """one gadget visit: its name and the bytes it reads (the gadget's letter
    once per layer unless given)"""
    g = GADGETS[name]
    letters = g.letters[0] * len(g.widths) if letters is None else letters
    assert len(letters) == len(g.widths) and set(letters) <= set(g.letters)
    return name, letters


def encode(visits, end=False):
    """x V1 x V2 x ... Vn x; with end=True without the last x (the last visit
    ends the string)"""
    assert visits or not end
    s = "x" + "x".join(l for _, l in visits)
    return (s if end or not visits else s + "x").encode()


class Case:
    """the automaton text, the packed corpus with pairwise distinct weights
    1 + sqrt(i + 2), and every string's visits"""

    def __init__(self, specs, pad=0):
        specs = [([visit(*((v,) if isinstance(v, str) else v)) for v in vs], end) for vs, end in specs]
        self.visits = [[n for n, _ in vs] for vs, _ in specs]
        self.strings = [encode(vs, end) for vs, end in specs]
        assert len(set(self.strings)) == len(self.strings), "a string twice"
        used = {n for vs in self.visits for n in vs}
        self.names = [n for n in GADGETS if n in used]   # (a state no string reaches would only be trimmed)
        self.text = wfsa_text(self.names, pad)
        self.sym = np.frombuffer(b"".join(self.strings), dtype=np.uint8).copy()
        self.off = np.concatenate([[0], np.cumsum([len(s) for s in self.strings])]).astype(np.int64)
        self.wt = 1.0 + np.sqrt(np.arange(len(self.strings)) + 2.0)
        assert len(np.unique(self.wt)) == len(self.wt)

    def traversal(self):
        """per string: it visits a gadget beyond the compile limits (the whole
        string then runs on the traversal path, its other bubbles with it)"""
        return np.array([any(GADGETS[n].klass == "trav" for n in vs) for vs in self.visits])

    def bubbles(self):
        """the gadgets of the compiled bubbles, string by string"""
        return [[GADGETS[n] for n in vs if GADGETS[n].klass] for vs, t in zip(self.visits, self.traversal()) if not t]

    def path_counts(self):
        return np.array([math.prod(GADGETS[n].paths for n in vs) for vs in self.visits], dtype=np.int64)

    def expected(self):
        """what stats() must report, from the visits alone"""
        flat = [g for bs in self.bubbles() for g in bs]
        return dict(small_bubbles_a=sum(g.klass == "A" for g in flat),
                    small_bubbles_b=sum(g.klass == "B" for g in flat),
                    big_bubbles=sum(g.klass == "big" for g in flat),
                    shaped_bubbles=sum(g.klass in "AB" and g.shape != 0 for g in flat),
                    fallback_strings=int(self.traversal().sum()),
                    max_bubble_nodes=max((g.nodes for g in flat), default=0),
                    max_bubble_edges=max((g.edges for g in flat), default=0))


def _both_positions(names):
    """every gadget mid-string and at the string's end, alone and behind a unary visit"""
    specs = []
    for n in names:
        specs += [([n], False), ([n], True), (["u1", n], True), (["v1", n], False)]
    return specs


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "all":
        # every gadget in both positions; the two-emission diamond on both letters of both states'
        # emissions; strings of several bubbles; no bubble at all; and the 33-node gadget, alone
        # and behind a diamond that goes to the traversal path with it
        specs = _both_positions(SMALL + BIG + LIMITS)
        specs += [([("m2", "l")], False), ([("m2", "l")], True)]
        specs += [(["d2", "t3", "c22"], False), (["d2", "s6"], False), (["t3", "s7"], True),
                  (["d2", "t3", "c33"], True), (["l1515", "d2"], False), (["f22", ("m2", "l"), "d2"], False)]
        specs += [([], False), (["u1"], False), (["v1", "u1"], True)]
        specs += [(["t1615"], False), (["t1615"], True), (["d2", "t1615"], False)]
        return Case(specs)
    if name == "big":
        return Case(_both_positions(BIG) + [([("m2", "l")], False), (["c33", "s7"], True), (["s6", "c2222"], False)])
    if name == "big1":   # the big bubbles of one-parameter edges alone: no multi-parameter edge in the model
        single = [n for n in BIG if not GADGETS[n].multi]
        return Case(_both_positions(single) + [(["c33", "s7"], True), (["s6", "c2222"], False)])
    if name == "limits":
        return Case(_both_positions(LIMITS))
    if name in LIMITS_PAD:   # the same corpus over an automaton of about 12,500 / 14,000 / 23,000 parameters
        return Case(_both_positions(LIMITS), pad=LIMITS_PAD[name])
    if name in ("mixed", "mixed_m2"):
        # one, two and three bubbles of mixed classes: A+B, A+big, B+big, A+B+big in both
        # orders and both positions (the per-string sums run in bubble order across the lists);
        # mixed_m2 with the two-emission diamond among them
        m2 = name == "mixed_m2"
        specs = _both_positions(["d2", "t3", "c22", "c33", "s7"] + ["m2"] * m2)
        for vs in (["d2", "t3"], ["t3", "d2"], ["d2", "s7"], ["c33", "d2"], ["c22", "s6"], ["s7", "q4"],
                   ["d2", "t3", "s6"], ["s7", "d2", "c22"], ["t3", ("m2", "l") if m2 else "c33", "d2"],
                   ["f22", "c2222", "d2"]):
            specs += [(vs, False), (vs, True)]
        return Case(specs)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def lanes(n):
    """n distinct strings around one identical class-A bubble (d2b,
    mid-string) and n around one identical class-B bubble (c22, mid-string):
    eight unary visits spell the string's number in u / v before the bubble.
    The lists are sorted by header, then by the edges' parameters.  Three
    (3,) bubbles sort before the (2,2) chains in the class-B list (fewer
    nodes: a smaller header), and three bubbles of the first diamond before
    the second one's in the class-A list (H's transitions into d2 have the
    smaller parameter numbers: LANES_FIRST, which the GPU test checks), so
    neither run of n starts at lane 0.  One bubble of each run's gadget at the
    string's end shares the run's parameters on its first edges only"""
    assert 1 <= n <= 256
    specs = []
    for i in range(n):
        prefix = [("u1", "v1")[i >> b & 1] for b in range(8)]
        specs += [(prefix + ["d2b"], False), (prefix + ["c22"], False)]
    specs += [(["t3"], False), (["t3"], True), (["u1", "t3"], False),
              (["d2"], False), (["d2"], True), (["v1", "d2"], False),
              (["d2b"], True), (["c22"], True), (["s6"], False)]
    return Case(specs)


LANES_FIRST = ("d2", "d2b")   # lanes(): every H -> d2 parameter is numbered before every H -> d2b parameter


# -- the reference -----------------------------------------------------------

SEEDS = (5, 6, 7)   # the weight draws: Init(7) plus perturbation(names, seed)


def get(key):
    """a corpus by name, or lanes(n) by its n"""
    return lanes(key) if isinstance(key, int) else case(key)


def perturbation(names, seed):
    """test_gpu_regimes._perturbation with a seed: rng.normal(0, 0.5) per
    trimmed parameter, by name -- the same move off the initial point for the
    learner and the oracle"""
    keys = sorted(names)
    return dict(zip(keys, np.random.default_rng(seed).normal(0.0, 0.5, size=len(keys))))


def oracle(key):
    from oracle import ENUM, Oracle
    c = get(key)
    return Oracle.from_arrays(c.text, c.sym, c.off, c.wt, mode=ENUM, max_paths=10_000_000)


def perturbed_oracle(key, seed):
    """(the ENUM oracle at Init(7) plus the seed's perturbation, its parameter names, the step by name)"""
    o = oracle(key)
    o.qn_init(7)
    names = o.param_names()
    step = perturbation(names, seed)
    o.set_x(o.x() + np.array([step[n] for n in names]))
    return o, names, step


@functools.lru_cache(maxsize=None)
def reference(key, seed):
    """the ENUM oracle's evaluation at the perturbed point, computed once and
    left unchanged: (step by name, KL, gradient in sorted-name order, log q
    per string)"""
    o, names, step = perturbed_oracle(key, seed)
    kl, _ = o.objective_grad()
    grad = dict(zip(names, o.grad()))
    grad_arr, logq = np.array([grad[n] for n in sorted(grad)]), o.logq()
    grad_arr.setflags(write=False)
    logq.setflags(write=False)
    return step, kl, grad_arr, logq


def oracle_rmin(o, x):
    """(smallest relative path probability over the ambiguous strings' paths,
    relative path probabilities, M's row pointers) at x, from the path
    matrices (test_gpu_regimes._oracle_rmin)"""
    prow, pcol, pdata, mrow = o.paths()
    path = np.repeat(np.arange(len(prow) - 1), np.diff(prow))
    lw = np.bincount(path, weights=pdata * x[pcol], minlength=len(prow) - 1)
    n_p = np.diff(mrow)
    assert n_p.min() >= 1
    e = np.exp(lw - np.repeat(np.maximum.reduceat(lw, mrow[:-1]), n_p))
    rpp = e / np.repeat(np.add.reduceat(e, mrow[:-1]), n_p)
    amb = np.where(np.repeat(n_p > 1, n_p), rpp, np.inf)
    return float(amb.min()), rpp, mrow
