"""Automata for the five wave-per-string trellis walkers, built by hand, and a
plain reference that knows paths as edge sequences
(test_trellis_gadgets_reference.py, test_gpu_trellis_gadgets.py) -- test
infrastructure, the sibling of bubble_gadgets.py, traversal_gadgets.py and
dense_gadgets.py for best_path_kernel, kbest_kernel<KC>, sample_path_kernel,
posterior_counts_kernel and marginal_rows_kernel / marginal_decode_kernel.

The walkers' other tests match a returned path to any oracle path of the same
parameter COUNT row; here a path is its sequence of in-edges and its end edge,
every edge that tells two paths apart carries a parameter, and the id list in
path order names the path (test_trellis_gadgets_reference.py asserts that per
case).  So the documented tie orders can be asserted path for path.

The layout.  Model reads the automaton through the library (Fsa.desc(): the
state order and each state's emission and transition order are the library's
-- its containers' iteration order, not the file's), hands the states in that
order to traversal_gadgets.fold() and restates the tier-2 table of wfsa_dev.hip
on the folded trellis (Wide): per byte the destinations ascending by node, each
once; a destination's in-edges in the order of a stable sort by destination of
(source node ascending, then the source's out-edge order); end edges per node
in ends[] order.  Which state sits in which lane is therefore read off the
table, never assumed from a name.

The cases (all weights by name; "zero" leaves every order to the ties):
(a) seam(w), w in 63, 64, 65, 128, 129: H fans out to w states that emit a, each
    back to H and to $; xa puts the seam into the end-edge scan, xaxa into the
    middle too.
(b) seam2(w0, w1, w2): three fully connected layers emitting c, a, b; every
    b-destination has w1 in-edges whose sources hold w0 prefixes each.
(c) ragged(): one b-destination with 70 in-edges beside 64 with one each;
    ragged_ends(): one node with 70 end edges beside 64 with one each.
(d) stale(): a string pair in which a score a wave left behind would change
    the next string's answer by 40, with strings that die at every stage.
(e) empty(): ^ has a transition into $: the empty string has one path.
(f) traversal_gadgets.composite(): parallel edges, edges of six parameters,
    chain nodes, composite end edges.
(g) few(m): exactly m paths.  (h) loop(): one path of 64 positions.
(i) ids65: seam(63) on xaxa puts counts on the parameter ids 63, 64 and 65."""
import fractions
import functools
import math

import numpy as np

import marginal_reference as MR
import sample_reference as SR
import traversal_gadgets as T
from bubble_gadgets import Gadget

START, END = T.START, T.END
NEG = -math.inf
SAMPLE_SEED = 20240917          # the one committed seed of the sampler replay
SAMPLE_MARGIN = 1e-9            # a draw is decidable when no running sum lies within this of u (relative to the total)
KS = (1, 2, 3, 4, 5, 8, 16)     # one k below, at and above every capacity of kbest_kernel<KC>
WAVE = 64


# -- the automaton in the library's numbering ---------------------------------------

def desc_states(fsa):
    """the states (name, emissions, transitions) in Fsa.desc()'s order, $ left out"""
    m = MR.model(fsa)
    names = fsa.state_names()
    out = []
    for u, name in enumerate(names):
        if u == m["end"]:
            assert m["em_ptr"][u] == m["em_ptr"][u + 1] and m["tr_ptr"][u] == m["tr_ptr"][u + 1]
            continue
        em = [m["em"][e][0].decode("latin-1") for e in range(m["em_ptr"][u], m["em_ptr"][u + 1])]
        tr = [names[m["tr"][t][0]] for t in range(m["tr_ptr"][u], m["tr_ptr"][u + 1])]
        out.append((name, em, tr))
    return out


class Wide:
    """the tier-2 table of wfsa_dev.hip restated on fold()'s trellis: node
    numbers (fold's order: the states, $, then the chain nodes by emission),
    slots[c] the destinations of byte c ascending, ins[c][k] the in-edges
    (e, source, parameters) of slot k with e counted through all bytes in
    ascending byte order, ends[node] its end edges (x, parameters) with x
    counted through the nodes, owner[node] the state a node belongs to"""

    def __init__(self, tr):
        self.nodes = list(tr.nodes)
        idx = {n: i for i, n in enumerate(self.nodes)}
        self.start = idx[START]
        self.n_states = self.nodes.index(END) + 1
        self.owner = [n[0] if isinstance(n, tuple) else n for n in self.nodes]
        by = {}
        for u in self.nodes:   # ascending source, each source's out-edges in fold's order
            for b, v, p in tr.edges[u]:
                by.setdefault(ord(b), []).append((idx[v], idx[u], tuple(p)))
        self.slots, self.ins = {}, {}
        e = 0
        for c in sorted(by):
            self.slots[c], self.ins[c] = [], []
            for dst, src, p in sorted(by[c], key=lambda t: t[0]):   # (stable)
                if not self.slots[c] or self.slots[c][-1] != dst:
                    self.slots[c].append(dst)
                    self.ins[c].append([])
                self.ins[c][-1].append((e, src, p))
                e += 1
        self.n_in_edges = e
        self.ends, x = {}, 0
        for u in self.nodes:
            self.ends[idx[u]] = []
            for p in tr.ends[u]:
                self.ends[idx[u]].append((x, tuple(p)))
                x += 1
        self.out = {}   # (byte, source) -> [(e, slot, destination)]
        for c in self.slots:
            for k, dst in enumerate(self.slots[c]):
                for e, src, _ in self.ins[c][k]:
                    self.out.setdefault((c, src), []).append((e, k, dst))

    def live(self, s, i):
        """the nodes live at position i of s, in slot order"""
        return [self.start] if i == 0 else self.slots.get(s[i - 1], [])


class Model:
    def __init__(self, states):
        import wfsa_amd as W
        self.text = T.wfsa_text(states)
        self.fsa = W.Fsa.read_text(self.text)
        self.states = desc_states(self.fsa)
        assert sorted(n for n, _, _ in self.states) == sorted(n for n, _, _ in states)
        self.trellis = T.fold(self.states)
        self.wide = Wide(self.trellis)
        self.names = self.fsa.param_names()          # parameter id -> (state, kind, label)
        self.pid = {n: j for j, n in enumerate(self.names)}
        assert sorted(self.names) == sorted(T.param_names(states))
        self.state_names = self.fsa.state_names()
        self.sid = {n: u for u, n in enumerate(self.state_names)}

    def weights(self, named=None, seed=None):
        """w_full: rng.normal(-1.2, 0.6) per parameter by sorted name (0 without a seed), then `named` on top"""
        from test_gpu_byte_marginals import fixture_weights
        w = fixture_weights(self.fsa, named)
        if seed is not None:
            draw = dict(zip(sorted(self.names), np.random.default_rng(seed).normal(-1.2, 0.6, size=len(self.names))))
            w = np.array([(named or {}).get(n, draw[n]) for n in self.names])
        w.setflags(write=False)
        return w

    def graded(self):
        """exact binary weights with many ties: -((j mod 7) / 8 + (j mod 3) / 4) by the parameter's rank in sorted names"""
        rank = {n: j for j, n in enumerate(sorted(self.names))}
        return self.weights({n: -((rank[n] % 7) / 8.0 + (rank[n] % 3) / 4.0) for n in self.names})


# -- the reference of one string ---------------------------------------------------------

class Path:
    __slots__ = ("edges", "x", "nodes", "ids", "lw")

    def __init__(self, edges, x, nodes, ids, lw):
        self.edges, self.x, self.nodes, self.ids, self.lw = edges, x, nodes, ids, lw


class Ref:
    """everything about one string at one w_full: the paths, the orders, the
    exact posterior, the MEA decode and the sampler's replay"""

    def __init__(self, model, s, w):
        self.model, self.s, self.L = model, bytes(s), len(s)
        wd = model.wide
        pid = model.pid

        def lw_of(params):   # one sum in list order from 0, as decode_edge_weight_kernel
            t = 0.0
            for p in params:
                t += float(w[pid[p]])
            return t
        self.lw_in = {}    # e -> (lw, ids)
        for c in set(self.s):
            for k in range(len(wd.slots.get(c, []))):
                for e, _, p in wd.ins[c][k]:
                    self.lw_in[e] = (lw_of(p), tuple(pid[q] for q in p))
        self.lw_end = {x: (lw_of(p), tuple(pid[q] for q in p)) for u in wd.ends for x, p in wd.ends[u]}
        self.paths = self._enumerate()
        self.index = {(p.edges, p.x): l for l, p in enumerate(self.paths)}
        self.finite = [l for l, p in enumerate(self.paths) if p.lw > NEG]

    # enumerate(string): every accepting path as (in-edges, end edge) with its ids in path order and its
    # weight, the one left-to-right sum of lw over the positions 0 .. L
    def _enumerate(self):
        wd, s, L = self.model.wide, self.s, self.L
        out = []

        def go(i, node, edges, nodes, ids, v):
            if i == L:
                for x, _ in wd.ends[node]:
                    out.append(Path(tuple(edges), x, tuple(nodes), tuple(ids + list(self.lw_end[x][1])), v + self.lw_end[x][0]))
                return
            for e, _, dst in wd.out.get((s[i], node), []):
                go(i + 1, dst, edges + [e], nodes + [dst], ids + list(self.lw_in[e][1]), v + self.lw_in[e][0])
        go(0, wd.start, [], [], [], 0.0)
        return out

    # -- the decoders' total order (decode.hpp) ----------------------------------------
    @functools.cached_property
    def order(self):
        """the finite-weight paths (indices into paths) in the K-best total
        order: a node's prefixes by (weight descending, in-edge ascending,
        source rank ascending), at the end by (weight descending, live slot
        ascending, end edge ascending, rank ascending); no K anywhere"""
        wd, s, L = self.model.wide, self.s, self.L
        lists = [{wd.start: [(0.0, None)]}]   # per position: node -> [(weight, (e, source, rank))] in order
        for i in range(L):
            cur, nxt = lists[-1], {}
            for k, dst in enumerate(wd.slots.get(s[i], [])):
                cand = []
                for e, src, _ in wd.ins[s[i]][k]:
                    lw = self.lw_in[e][0]
                    for r, (v, _) in enumerate(cur.get(src, [])):
                        if v + lw > NEG:
                            cand.append((-(v + lw), e, r, src))
                cand.sort()
                if cand:
                    nxt[dst] = [(-nv, (e, src, r)) for nv, e, r, src in cand]
            lists.append(nxt)
        final = []
        for k, node in enumerate(wd.live(s, L)):
            for x, _ in wd.ends[node]:
                for r, (v, _) in enumerate(lists[L].get(node, [])):
                    if v + self.lw_end[x][0] > NEG:
                        final.append((-(v + self.lw_end[x][0]), k, x, r, node))
        final.sort()
        out = []
        for nv, _, x, r, node in final:
            edges = []
            for i in range(L, 0, -1):
                e, node, r = lists[i][node][r][1]
                edges.append(e)
            l = self.index[(tuple(reversed(edges)), x)]
            assert self.paths[l].lw == -nv, "the DP's weight is the path's one left-to-right sum"
            out.append(l)
        assert sorted(out) == self.finite
        return out

    # -- the exact posterior ------------------------------------------------------------------
    @functools.cached_property
    def posterior(self):
        """logq, prob (per path; exact fractions where every finite weight is
        0), counts {parameter id: expected count}, entropy, mass[i] {state
        id: mass}, boundary[i]; logq -inf: nothing else"""
        P = [self.paths[l] for l in self.finite]
        if not P:
            return dict(logq=NEG)
        if all(p.lw == 0.0 for p in P):
            prob = [fractions.Fraction(1, len(P))] * len(P)
            logq, add = math.log(len(P)), sum
            ent = math.log(len(P))
        else:
            m = max(p.lw for p in P)
            logq = m + math.log(math.fsum(math.exp(p.lw - m) for p in P))
            prob = [math.exp(p.lw - logq) for p in P]
            add = math.fsum
            ent = -math.fsum(q * (p.lw - logq) for q, p in zip(prob, P)) if len(P) > 1 else 0.0
        if len(P) == 1:
            prob = [fractions.Fraction(1)]
            add = sum
        wd, sid = self.model.wide, self.model.sid
        terms = {}
        for q, p in zip(prob, P):
            for j in p.ids:
                terms.setdefault(j, []).append(q)
        counts = {j: float(add(v)) for j, v in terms.items()}
        mass, boundary = [], []
        for i in range(self.L):
            per, ends = {}, []
            for q, p in zip(prob, P):
                node = p.nodes[i]
                per.setdefault(sid[wd.owner[node]], []).append(q)
                if node < wd.n_states:
                    ends.append(q)
            mass.append({u: float(add(v)) for u, v in per.items()})
            boundary.append(float(add(ends)) if ends else 0.0)
        return dict(logq=logq, prob=[float(q) for q in prob], counts=counts, entropy=ent, mass=mass, boundary=boundary)

    # -- the MEA decode (marginals.hpp) ----------------------------------------------------------
    def mea(self, mass):
        """(path index, score) of the max-expected-accuracy decode under the
        per-byte state masses mass[i][state id] (the exact ones, or the ones a
        device stored): a destination's score is its best eligible in-edge's
        source score plus its own mass, in-edges by (source score descending,
        lw descending, e ascending); at the end (score descending, node
        ascending) over the live nodes with a finite end edge, then (lw
        descending, end edge ascending).  None: no path of finite weight"""
        wd, s, L, sid = self.model.wide, self.s, self.L, self.model.sid
        if not self.finite:
            return None
        score, back = [{wd.start: 0.0}], [{}]
        for i in range(L):
            cur, nxt, bp = score[-1], {}, {}
            for k, dst in enumerate(wd.slots.get(s[i], [])):
                best = None
                for e, src, _ in wd.ins[s[i]][k]:
                    lw = self.lw_in[e][0]
                    if src not in cur or not (NEG < lw < math.inf):
                        continue
                    key = (-cur[src], -lw, e)
                    if best is None or key < best[0]:
                        best = (key, e, src)
                if best is not None:
                    nxt[dst] = cur[best[2]] + float(mass[i].get(sid[wd.owner[dst]], 0.0))
                    bp[dst] = (best[1], best[2])
            score.append(nxt)
            back.append(bp)
        best = None
        for node in wd.live(s, L):
            if node not in score[L]:
                continue
            fin = [(-self.lw_end[x][0], x) for x, _ in wd.ends[node] if NEG < self.lw_end[x][0] < math.inf]
            if fin and (best is None or (-score[L][node], node) < best[0]):
                best = ((-score[L][node], node), min(fin)[1], node)
        if best is None:
            return None
        _, x, node = best
        total, edges = score[L][node], []
        for i in range(L, 0, -1):
            e, node = back[i][node]
            edges.append(e)
        return self.index[(tuple(reversed(edges)), x)], total

    def mea_score(self, l, mass):
        """the score of path l: its bytes' masses added left to right"""
        wd, sid, t = self.model.wide, self.model.sid, 0.0
        for i, node in enumerate(self.paths[l].nodes):
            t += float(mass[i].get(sid[wd.owner[node]], 0.0))
        return t

    # -- the sampler's replay (sample.hip) -----------------------------------------------------------
    @functools.cached_property
    def alpha(self):
        """the forward rows as sample.hip forms them: per position i >= 1 the log
        alpha of every slot, the greatest term plus the log of the sum of
        exp(term - greatest) in e_ptr order; None from the position nothing reaches"""
        wd, s = self.model.wide, self.s
        rows, cur = [None], {wd.start: 0.0}
        for i in range(self.L):
            row, nxt = [], {}
            for k, dst in enumerate(wd.slots.get(s[i], [])):
                terms = [cur.get(src, NEG) + self.lw_in[e][0] for e, src, _ in wd.ins[s[i]][k]]
                mx = max(terms)
                t = NEG
                if mx > NEG:
                    tot = 0.0
                    for v in terms:
                        tot += math.exp(v - mx)
                    t = mx + math.log(tot)
                    nxt[dst] = t
                row.append(t)
            if not nxt:
                return rows + [None] * (self.L - i)
            rows.append(row)
            cur = nxt
        return rows

    @staticmethod
    def _choose(masses, u):
        """the kernel's choice among `masses` for the draws u: the running sums c
        against u * total, the last positive mass at or before the first c >
        target; (index per draw, -1: none; decidable per draw)"""
        c = np.cumsum(np.array(masses, dtype=np.float64))   # (sequential, as the kernel adds)
        total = c[-1]
        target = u * total
        first = np.minimum(np.searchsorted(c, target, side="right"), len(c) - 1)
        last_pos = np.full(len(c), -1)
        at = -1
        for j, m in enumerate(masses):
            if m > 0.0:
                at = j
            last_pos[j] = at
        clear = np.abs(c[None, :] - target[:, None]).min(axis=1) > SAMPLE_MARGIN * total
        return last_pos[first], clear

    def replay(self, U):
        """the walks of the draws U[M, L + 1] (column d: draw d, 0 at the end and
        L + 1 - i for the in-edge into position i): (path index per walk, all
        its draws decidable).  log q as the kernel forms it is self.sample_logq"""
        wd, s, L = self.model.wide, self.s, self.L
        M = len(U)
        rows = self.alpha
        assert self.finite and (L == 0 or rows[L] is not None)
        live = wd.live(s, L)
        items = [(k, x, (rows[L][k] if L else 0.0) + self.lw_end[x][0]) for k, node in enumerate(live) for x, _ in wd.ends[node]]
        mx = max(v for _, _, v in items)
        pick, ok = self._choose([math.exp(v - mx) for _, _, v in items], U[:, 0])
        assert (pick >= 0).all()
        X = np.array([x for _, x, _ in items])[pick]
        K = np.array([k for k, _, _ in items])[pick]
        E = np.zeros((M, L), dtype=np.int64)
        for i in range(L, 0, -1):
            c = s[i - 1]
            newK = np.zeros(M, dtype=np.int64)
            for k in np.unique(K):
                sel = np.flatnonzero(K == k)
                la = rows[i][k]
                prev = wd.live(s, i - 1)
                masses, srcs = [], []
                for e, src, _ in wd.ins[c][k]:
                    if i < 2:
                        las = 0.0 if src == wd.start else NEG
                    else:
                        las = rows[i - 1][prev.index(src)] if src in prev else NEG
                    masses.append(math.exp(las + self.lw_in[e][0] - la))
                    srcs.append(prev.index(src) if src in prev else 0)
                pick, clear = self._choose(masses, U[sel, L + 1 - i])
                assert (pick >= 0).all()
                ok[sel] &= clear
                E[sel, i - 1] = np.array([e for e, _, _ in wd.ins[c][k]])[pick]
                newK[sel] = np.array(srcs)[pick]
            K = newK
        rowsE, inv = np.unique(np.concatenate([E, X[:, None]], axis=1), axis=0, return_inverse=True)
        which = np.array([self.index[(tuple(int(v) for v in r[:-1]), int(r[-1]))] for r in rowsE])
        return which[np.asarray(inv).reshape(-1)], ok

    @functools.cached_property
    def sample_logq(self):
        """log q over the end edges in (live slot, end edge) order, as the three (+, x) kernels form it"""
        wd, s, L = self.model.wide, self.s, self.L
        rows = self.alpha
        if L and rows[L] is None:
            return NEG
        v = [(rows[L][k] if L else 0.0) + self.lw_end[x][0] for k, node in enumerate(wd.live(s, L)) for x, _ in wd.ends[node]]
        mx = max(v, default=NEG)
        if not mx > NEG:
            return NEG
        tot = 0.0
        for t in v:
            tot += math.exp(t - mx)
        return mx + math.log(tot)


def draws(seed, strings, n, L):
    """U[len(strings) * n, L + 1]: the uniforms of samples 0 .. n - 1 of the strings with these corpus indices"""
    sid = np.repeat(np.asarray(strings, dtype=np.uint64), n).reshape(-1, 1)
    smp = np.tile(np.arange(n, dtype=np.uint64), len(strings)).reshape(-1, 1)
    return SR.uniforms(seed, sid, smp, L + 1)


# -- the cases ------------------------------------------------------------------------------------------

class Case:
    """a model, its corpus (strings may repeat) and its named weightings"""

    def __init__(self, name, model, strings, weightings):
        self.name, self.model, self.strings, self.weightings = name, model, [bytes(s) for s in strings], weightings
        self.sym = np.frombuffer(b"".join(self.strings), dtype=np.uint8).copy()
        self.off = np.concatenate([[0], np.cumsum([len(s) for s in self.strings])]).astype(np.int64)
        self.distinct = list(dict.fromkeys(self.strings))
        self._refs = {}

    def ref(self, weighting, s):
        """the reference of one string alone, computed once and left unchanged"""
        key = (weighting, bytes(s))
        if key not in self._refs:
            self._refs[key] = Ref(self.model, s, self.weightings[weighting])
        return self._refs[key]


def layered(name, letters, widths):
    """fully connected layers behind H, layer i emitting letters[i]; the last layer -> H and $"""
    g = Gadget(name, "".join(letters), widths)
    out = []
    for i, w in enumerate(widths):
        nxt = [g.state(i + 1, m) for m in range(widths[i + 1])] if i + 1 < len(widths) else ["H", END]
        out += [(g.state(i, j), [letters[i]], nxt) for j in range(w)]
    first = [g.state(0, j) for j in range(widths[0])]
    return [(START, [""], ["H"]), ("H", ["x"], first + [END])] + out


SEAMS = (63, 64, 65, 128, 129)


@functools.lru_cache(maxsize=None)
def seam(w):
    """zero: ties alone; raised: one weight up on the slot of index min(64, w - 1) of byte a, the first slot of
    lane 0's second round where there is one; graded: the weight grows with the slot, so the 16 best of xa are
    the slots w - 1 .. w - 16, across the round boundary; random: no ties"""
    m = Model(T.automaton([Gadget("s", "a", (w,))]))
    slots = [m.wide.nodes[n] for n in m.wide.slots[ord("a")]]
    assert len(slots) == w
    weightings = {"zero": m.weights(), "raised": m.weights({("H", "T", slots[min(64, w - 1)]): 1.0}),
                  "graded": m.weights({("H", "T", n): 0.25 * j for j, n in enumerate(slots)}), "random": m.weights(seed=w)}
    return Case(f"seam{w}", m, [b"xa", b"xaxa"], weightings)


SEAM2 = ((2, 65, 64), (16, 3, 65), (16, 64, 2))


@functools.lru_cache(maxsize=None)
def seam2(w0, w1, w2):
    m = Model(layered("t", "cab", (w0, w1, w2)))
    return Case(f"seam2_{w0}_{w1}_{w2}", m, [b"xcab", b"xcabx"], {"zero": m.weights(), "graded": m.graded(), "random": m.weights(seed=w1)})


def _ragged_states(heavy):
    a = [(f"A{j}", ["a"], [heavy, f"B{j}"] if j < 64 else [heavy, END]) for j in range(70)]
    b = [(f"B{j}", ["b"], ["H", END]) for j in range(64)]
    return [(START, [""], ["H"]), ("H", ["x"], [n for n, _, _ in a] + [END])] + a + [(heavy, ["b"], ["H", END])] + b


def _first_off_lane0(build, byte):
    """the first heavy-state name under which that state's slot among the byte's destinations is not lane 0's"""
    for name in ("Z", "Y", "W", "V", "U"):
        m = Model(build(name))
        if m.wide.slots[ord(byte)].index(m.wide.nodes.index(name)) % WAVE != 0:
            return m, name
    raise AssertionError("every candidate name lands in lane 0")


@functools.lru_cache(maxsize=None)
def ragged():
    """xab: the destinations of b are the heavy state (70 in-edges from 70
    live sources) and B0 .. B63 (one in-edge each); xabx merges their lists in H"""
    m, heavy = _first_off_lane0(_ragged_states, "b")
    c = Case("ragged", m, [b"xab", b"xabx"], {"zero": m.weights(), "graded": m.graded(), "random": m.weights(seed=70)})
    c.heavy = heavy
    return c


def _ragged_end_states(heavy):
    n = [(f"N{j}", [""], [END]) for j in range(70)]
    b = [(f"B{j}", ["a"], ["H", END]) for j in range(64)]
    return [(START, [""], ["H"]), ("H", ["x"], [heavy] + [s for s, _, _ in b] + [END]),
            (heavy, ["a"], [s for s, _, _ in n])] + n + b


@functools.lru_cache(maxsize=None)
def ragged_ends():
    """xa: the heavy state has 70 end edges (over 70 epsilon states), B0 .. B63 one each"""
    m, heavy = _first_off_lane0(_ragged_end_states, "a")
    c = Case("ragged_ends", m, [b"xa"], {"zero": m.weights(), "graded": m.graded(), "random": m.weights(seed=71)})
    c.heavy = heavy
    return c


STALE_GAP = 40.0
STALE_STATES = [(START, [""], ["H", "P"]), ("H", ["x"], ["P", "D", END]), ("P", ["a", "c"], ["Q", "Q2", "T"]),
                ("Q", ["b"], ["T", END]), ("Q2", ["b"], ["T", "H"]), ("T", ["c"], [END, "H"]), ("D", ["d"], [END, "H"])]
# P is entered by a (from ^ and from H) and by c; T by c from P, Q and Q2.  In xabc the sources of byte c's
# in-edges are read in the row of position 3, where only Q and Q2 are live; ac leaves P in that row's parity
# (position 1).  P -> T weighs STALE_GAP more than the rest, so a P left finite takes everything over.
STALE_CYCLE = [b"ac", b"xabc", b"xac", b"xabc", b"az", b"xabc", b"aa", b"xabc", b"a", b"xabc", b"xaz", b"xabc",
               b"xd", b"xabc", b"", b"xabc", b"xabcx", b"xabc", b"aba", b"xabc", b"abc", b"xab", b"b", b"xabc"]
STALE_N = 3 * 4096 + 12


@functools.lru_cache(maxsize=None)
def stale():
    """3 x 4096 + 12 strings on at most 4,096 waves: about three per wave.  az and xaz hold a byte without a
    destination, b dies at position 1, aa at position 2, aba at its last byte, a reaches the end on a node
    without an end edge, xd's only path weighs -inf, and the empty string has no path here (^ has no end edge)"""
    m = Model(STALE_STATES)
    named = {("P", "T", "T"): STALE_GAP, ("H", "T", "D"): NEG}
    strings = [STALE_CYCLE[i % len(STALE_CYCLE)] for i in range(STALE_N)]
    return Case("stale", m, strings, {"random": m.weights(named, seed=40)})


EMPTY_STATES = [(START, [""], ["H", END]), ("H", ["x"], ["e_0_0", "e_0_1", END]),
                ("e_0_0", ["a"], ["H", END]), ("e_0_1", ["a"], ["H", END])]


@functools.lru_cache(maxsize=None)
def empty(alone=False):
    m = Model(EMPTY_STATES)
    strings = [b""] if alone else [b"", b"xa", b"", b"x", b"xaxa", b""]
    return Case("empty_alone" if alone else "empty", m, strings, {"zero": m.weights(), "random": m.weights(seed=5)})


COMPOSITE_MAX_PATHS = 1000


@functools.lru_cache(maxsize=None)
def composite():
    """traversal_gadgets.composite() with its strings of at most 1,000 paths (the rejected ones included)"""
    c = T.composite()
    m = Model(c.states)
    strings = [s for s, n in zip(c.strings, c.paths) if n <= COMPOSITE_MAX_PATHS]
    return Case("composite", m, strings, {"zero": m.weights(), "graded": m.graded(), "random": m.weights(seed=11)})


@functools.lru_cache(maxsize=None)
def few(n):
    m = Model(T.automaton([Gadget("f", "a", (n,))]))
    return Case(f"few{n}", m, [b"xa"], {"zero": m.weights(), "random": m.weights(seed=n)})


LOOP_LEN = 64


@functools.lru_cache(maxsize=None)
def loop():
    m = Model(T.automaton([], h_extra=["H"]))
    return Case("loop", m, [b"x" * LOOP_LEN], {"random": m.weights(seed=64)})


def ids65():
    """(the case, the weighting, the string) whose posterior has counts on the parameter ids 63, 64 and 65"""
    return seam(63), "random", b"xaxa"


CASES = {f"seam{w}": functools.partial(seam, w) for w in SEAMS}
CASES.update({"seam2_%d_%d_%d" % t: functools.partial(seam2, *t) for t in SEAM2})
CASES.update(ragged=ragged, ragged_ends=ragged_ends, stale=stale, empty=empty, empty_alone=functools.partial(empty, True),
             composite=composite, few1=functools.partial(few, 1), few3=functools.partial(few, 3), loop=loop)


def clear_caches():
    for f in (seam, seam2, ragged, ragged_ends, stale, empty, composite, few, loop):
        f.cache_clear()
