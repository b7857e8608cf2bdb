"""Automata for the dense path (dense_path.hip, dense_decode.hip) built by
hand, with their corpora, a long-double reference and the row-slot rule
restated (test_dense_gadgets_reference.py, test_gpu_dense_gadgets.py) -- test
infrastructure, the sibling of bubble_gadgets.py and traversal_gadgets.py.

Every other dense test loads Synthetic(dense=True): every S -> T, ^ -> T and
T -> $ edge present, no ^ -> $, no parameter-free edge, every string from a
walk.  The gadgets here have

  * holes: absent entries of A, of the start row and of the end column
    (kCodeNone), single-member groups (kCodeOne), a ^ -> $ edge, strings that
    die mid-way or at the end, the empty string (holes12);
  * states on both sides of a column-tile edge (edge127 / 128 / 129), three
    column tiles (tiles384), two, three and four row tiles chosen on purpose
    (rows256, tiles384, xcd512), T = 1 and T = 2 (t1, xcd512), one string in
    127 idle rows (single), many strings per slot with runs of length-1
    strings (seams);
  * vocabularies past one window of dense_reduce_kernel (vocab65, vocab94,
    vocab130: a second window partly and exactly full, a third);
  * a total log weight near -12000 (long300) and posteriors of 4e-18 next to
    1 (peaked).

A gadget is a function returning Gadget(text, sym, off, p, R, T, notes): the
automaton in traversal_gadgets.wfsa_text's format (all weights 0; the weights
of a test come from weights()), the packed corpus, p = weight / sum, the row
slots and steps load_corpus must choose, and what the gadget promises.

reference() is the plain restatement in numpy.longdouble, per string, that
the device is held to; restate() is a float64 one laid out as the device
(row slots, column tiles, vocabulary windows) that measures what float64
costs and takes one injected fault at a time."""
import functools
import heapq
import itertools
from typing import NamedTuple

import numpy as np

from traversal_gadgets import END, START, wfsa_text

LD = np.longdouble
TILE = 128          # kDenseTile: rows per row tile, columns per column tile
RED_WINDOW = 64     # kRedWindow: symbols per LDS pass of dense_reduce_kernel
N_CU = 256          # the cost rule's divisor; every corpus here keeps (R/128)(np/128) <= 16 blocks per step


class Gadget(NamedTuple):
    text: str
    sym: np.ndarray
    off: np.ndarray
    p: np.ndarray
    R: int
    T: int
    notes: dict


# -- the row-slot rule ---------------------------------------------------------

def slot_shape(lengths, np_, n_cu=N_CU):
    """DensePath::load_corpus restated: (R, T, slots).  R is the first
    multiple of 128 (up to the one that gives every non-empty string a slot
    of its own) with the fewest step-rounds max(t - 1, 1) ceil(blocks / CUs),
    t = max(longest, ceil(symbols / R)); the non-empty strings then go
    longest first (ties in corpus order) onto the least loaded slot (ties to
    the lower slot); T is the fullest slot's load"""
    lengths = [int(x) for x in lengths]
    order = [i for i, n in enumerate(lengths) if n > 0]
    total, lmax = sum(lengths), max(lengths, default=0)
    nct = np_ // TILE
    R, best = TILE, None
    for k in range(1, max(1, -(-len(order) // TILE)) + 1):
        r = k * TILE
        t = max(lmax, -(-total // r))
        cost = max(t - 1, 1) * (-(-(k * nct) // n_cu))
        if best is None or cost < best - 1e-9:
            best, R = cost, r
    order.sort(key=lambda i: -lengths[i])   # (stable)
    heap = [(0, r) for r in range(R)]
    slots = [[] for _ in range(R)]
    for i in order:
        load, r = heapq.heappop(heap)
        slots[r].append(i)
        heapq.heappush(heap, (load + lengths[i], r))
    T = max(1, max(sum(lengths[i] for i in s) for s in slots))
    return R, T, slots


# -- comparison ------------------------------------------------------------------

def close(got, want, rel, atol=0.0):
    """every entry: |got - want| <= max(atol, rel max(|got|, |want|)); an
    infinite entry equals only itself, a NaN nothing"""
    g, w = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD)
    if g.shape != w.shape:
        return False
    fin = np.isfinite(g) & np.isfinite(w)
    if not np.array_equal(g[~fin], w[~fin]):   # (NaN != NaN)
        return False
    g, w = g[fin], w[fin]
    return bool(np.all(np.abs(g - w) <= np.maximum(LD(atol), LD(rel) * np.maximum(np.abs(g), np.abs(w)))))


def distance(got, want, atol=0.0):
    """the smallest rel at which close(got, want, rel, atol) holds (inf: none)"""
    g, w = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD)
    fin = np.isfinite(g) & np.isfinite(w)
    if g.shape != w.shape or not np.array_equal(g[~fin], w[~fin]):
        return float("inf")
    g, w = g[fin], w[fin]
    d = np.abs(g - w)
    m = d > LD(atol)
    return float(np.max(d[m] / np.maximum(np.abs(g[m]), np.abs(w[m])))) if m.any() else 0.0


# the dense tests' own bounds (test_gpu_dense.py)
LOGQ_REL, GRAD_REL, GRAD_ATOL, RMIN_REL = 1e-12, 1e-10, 1e-17, 1e-11
ORDER_FACTOR = 16.0   # another, equally valid order of a sum over <= 384 columns
LOOSENED = ("long300", "peaked", "tiles384")


def bounds(name, f64):
    """(log q and LL rel, gradient rel, rmin rel) of a gadget: the project's
    bounds; for the gadgets in LOOSENED the larger of each and 16 times the
    distance f64 = (log q, gradient, rmin) of restate() from reference()"""
    if name not in LOOSENED:
        return LOGQ_REL, GRAD_REL, RMIN_REL
    return tuple(max(b, ORDER_FACTOR * d) for b, d in zip((LOGQ_REL, GRAD_REL, RMIN_REL), f64))


# -- reference -------------------------------------------------------------------

class Result(NamedTuple):
    logq: np.ndarray      # [S]  log q, -inf for a dead string
    ll: float             # sum of p log q over the strings with p > 0
    grad: np.ndarray      # [n_params]  -sum p E[count]
    rmin: np.ndarray      # [S]  smallest relative path probability (nan: dead)
    paths: list           # [S]  accepting paths, Python integers
    used: np.ndarray      # [n_params]  on an accepting path of some string


def _weights_of(par, w, dtype):
    """exp-weights of a code table: exp(w[code]), 1 for a single-member group, 0 for no edge"""
    e = np.exp(np.asarray(w, dtype=dtype))
    return np.where(par >= 0, e[np.maximum(par, 0)], np.where(par == -1, dtype(1), dtype(0)))


def _logs_of(par, w):
    """log weights for the (min, +) pass: +inf for no edge"""
    w = np.asarray(w, dtype=LD)
    return np.where(par >= 0, w[np.maximum(par, 0)], np.where(par == -1, LD(0), LD(np.inf)))


def _scatter(n_params, tab, CA, CE, C0, Cend, Cse, dtype):
    g = np.zeros(n_params, dtype=dtype)
    for par, cnt in ((tab.pA, CA), (tab.pE, CE), (tab.p0, C0), (tab.pend, Cend)):
        ok = par >= 0
        np.add.at(g, par[ok], -cnt[ok])
    if tab.pse >= 0:
        g[tab.pse] -= Cse
    return g


def reference(fsa, w, sym, off, p):
    """every string on its own, in numpy.longdouble: a forward pass scaled at
    every position, the backward pass in the same scales, the posterior counts
    of every edge; a (min, +) pass over the log weights; the accepting paths
    by integer DP over the present edges"""
    from dense_decode_reference import Tables
    tab = Tables(fsa, w)
    n, S = tab.n, len(off) - 1
    n_params = len(np.asarray(w))
    A, E, a0, aend = (_weights_of(t, w, LD) for t in (tab.pA, tab.pE, tab.p0, tab.pend))
    se = _weights_of(np.array([tab.pse]), w, LD)[0]
    lA, lE, l0, lend = (_logs_of(t, w) for t in (tab.pA, tab.pE, tab.p0, tab.pend))
    mA, mE, m0, mend = tab.pA != -2, tab.pE != -2, tab.p0 != -2, tab.pend != -2
    lmax = int(np.max(np.diff(off))) if S else 0
    big = float(n) ** max(lmax, 1) >= 2.0 ** 62
    iA = mA.astype(object if big else np.int64)
    CA, CE, C0, Cend, Cse = np.zeros((n, n), LD), np.zeros((n, 256), LD), np.zeros(n, LD), np.zeros(n, LD), LD(0)
    UA, UE, U0, Uend, Use = np.zeros((n, n), bool), np.zeros((n, 256), bool), np.zeros(n, bool), np.zeros(n, bool), False
    logq, rmin, paths = np.full(S, -np.inf, LD), np.full(S, np.nan, LD), []
    for i in range(S):
        s = np.asarray(sym[off[i]:off[i + 1]], dtype=np.int64)
        L = len(s)
        if L == 0:
            paths.append(int(tab.pse != -2))
            if tab.pse != -2:
                logq[i], rmin[i] = np.log(se), LD(1)
                Cse += LD(p[i])
                Use = True
            continue
        # accepting paths
        c = (m0 & mE[:, s[0]]).astype(iA.dtype)
        for b in s[1:]:
            c = c.dot(iA) * mE[:, b].astype(iA.dtype)
        paths.append(int((c * mend.astype(iA.dtype)).sum()))
        # scaled forward
        al, z = np.zeros((L, n), LD), np.zeros(L, LD)
        a = a0 * E[:, s[0]]
        for j in range(L):
            if j:
                a = al[j - 1].dot(A) * E[:, s[j]]
            z[j] = a.sum()
            if not z[j] > 0:
                break
            al[j] = a / z[j]
        fin = al[L - 1].dot(aend)
        if not fin > 0:
            assert paths[-1] == 0
            continue
        assert paths[-1] > 0
        logq[i] = np.log(z).sum() + np.log(fin)
        # backward, in the scale where al[j] * be sums to 1
        pi = LD(p[i])
        be = aend / fin
        Cend += pi * al[L - 1] * be
        Uend |= (al[L - 1] > 0) & mend
        reach = (al[L - 1] > 0) & mend       # states at j on an accepting path
        for j in range(L - 1, -1, -1):
            CE[:, s[j]] += pi * al[j] * be
            UE[:, s[j]] |= reach
            if j == 0:
                C0 += pi * al[0] * be
                U0 |= reach
                break
            nxt = E[:, s[j]] * be / z[j]
            CA += pi * np.outer(al[j - 1], nxt) * A
            edge = np.outer(al[j - 1] > 0, reach) & mA
            UA |= edge
            reach = edge.any(axis=1)
            be = A.dot(nxt)
        # the lightest accepting path
        m = l0 + lE[:, s[0]]
        for b in s[1:]:
            m = np.min(m[:, None] + lA, axis=0) + lE[:, b]
        rmin[i] = np.exp(np.min(m + lend) - logq[i])
    pl = np.asarray(p, dtype=LD)
    live = pl > 0
    ll = float(np.sum(pl[live] * logq[live])) if live.any() else 0.0
    grad = _scatter(n_params, tab, CA, CE, C0, Cend, Cse, LD)
    used = _scatter(n_params, tab, UA.astype(LD), UE.astype(LD), U0.astype(LD), Uend.astype(LD), LD(Use), LD) < 0
    return Result(logq, ll, grad, rmin, paths, used)


# -- the float64 restatement, laid out as the device -----------------------------

FAULTS = ("last_tile", "start_as_continuation", "symbols_from_64", "no_start_end_edge", "dead_scale_leaks")


def restate(fsa, w, sym, off, p, fault=None):
    """float64, slot by slot as the device runs them (slot_shape): every
    string of a slot after the one before it, the row scale the sum of the
    column tiles' partial sums, the emission counts by vocabulary window.
    Returns (log q, LL, gradient, rmin per string).  fault injects one error:
      last_tile              a row's scale leaves out its last column tile (when there are several)
      start_as_continuation  a start row that follows another string takes alpha A as a continuation
      symbols_from_64        the emission sums skip the symbols past the first window
      no_start_end_edge      ^ -> $ is ignored
      dead_scale_leaks       the log scale of a dead string is carried into the next string of its slot"""
    from dense_decode_reference import Tables
    assert fault is None or fault in FAULTS
    tab = Tables(fsa, w)
    n, S = tab.n, len(off) - 1
    np_ = -(-n // TILE) * TILE
    nct = np_ // TILE
    f8 = np.float64
    A, E, a0, aend = (_weights_of(t, w, f8) for t in (tab.pA, tab.pE, tab.p0, tab.pend))
    se = 0.0 if fault == "no_start_end_edge" else _weights_of(np.array([tab.pse]), w, f8)[0]
    lA, lE, l0, lend = (_logs_of(t, w).astype(f8) for t in (tab.pA, tab.pE, tab.p0, tab.pend))
    sym_of_byte = np.cumsum((tab.pE != -2).any(axis=0)) - 1   # the used bytes in byte order

    def scale(a):
        parts = [a[c * TILE:(c + 1) * TILE].sum() for c in range(nct)]
        if fault == "last_tile" and nct > 1:
            parts = parts[:-1]
        return sum(parts)

    lengths = np.diff(off)
    _, _, slots = slot_shape(lengths, np_)
    CA, CE, C0, Cend, Cse = np.zeros((n, n)), np.zeros((n, 256)), np.zeros(n), np.zeros(n), 0.0
    logq, rmin = np.full(S, -np.inf), np.full(S, np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in np.flatnonzero(lengths == 0):
            logq[i] = np.log(se)
            if se > 0:
                rmin[i] = 1.0
                Cse += p[i]
        for slot in slots:
            prev, la_prev = None, 0.0    # the row before, scaled, and its log scale
            for i in slot:
                s = np.asarray(sym[off[i]:off[i + 1]], dtype=np.int64)
                L = len(s)
                al, z = np.zeros((L, n)), np.zeros(L)
                if fault == "start_as_continuation" and prev is not None:
                    a = prev.dot(A) * E[:, s[0]]
                else:
                    a = a0 * E[:, s[0]]
                la = la_prev if fault == "dead_scale_leaks" and la_prev == -np.inf else 0.0
                for j in range(L):
                    if j:
                        a = al[j - 1].dot(A) * E[:, s[j]]
                    z[j] = scale(a)
                    la += np.log(z[j])
                    al[j] = a / z[j] if z[j] > 0 else 0.0
                prev, la_prev = al[L - 1], la
                fin = al[L - 1].dot(aend)
                logq[i] = la + np.log(fin)
                if not logq[i] > -np.inf:
                    logq[i] = -np.inf
                    continue
                be = aend / fin
                Cend += p[i] * al[L - 1] * be
                for j in range(L - 1, -1, -1):
                    g = p[i] * al[j] * be
                    if not (fault == "symbols_from_64" and sym_of_byte[s[j]] >= RED_WINDOW):
                        CE[:, s[j]] += g
                    if j == 0:
                        C0 += g
                        break
                    nxt = E[:, s[j]] * be / z[j]
                    CA += p[i] * np.outer(al[j - 1], nxt) * A
                    be = A.dot(nxt)
                m = l0 + lE[:, s[0]]
                for b in s[1:]:
                    m = np.min(m[:, None] + lA, axis=0) + lE[:, b]
                rmin[i] = np.exp(np.min(m + lend) - logq[i])
    pv = np.asarray(p, dtype=f8)
    live = pv > 0
    ll = float(np.sum(pv[live] * logq[live])) if live.any() else 0.0
    return logq, ll, _scatter(len(np.asarray(w)), tab, CA, CE, C0, Cend, Cse, f8), rmin


# -- automata ------------------------------------------------------------------

ALPHABET = "".join(chr(b) for b in list(range(0x21, 0x7f)) + list(range(0xa1, 0x100)))   # no blank, no control byte


def weights(g, names):
    """the gadget's weight draw, by parameter name (names: Fsa.param_names()):
    normal(mean, sd) from its seed over the sorted names, then the weights the gadget sets itself"""
    seed, mean, sd = g.notes["draw"]
    keys = sorted(set(names))
    by_name = dict(zip(keys, np.random.default_rng(seed).normal(mean, sd, size=len(keys))))
    by_name.update(g.notes.get("set", {}))
    return np.array([by_name[nm] for nm in names])


def _names(n):
    return [f"s{i}" for i in range(n)]


def _states(names, mask, start_to, end_from, emis, start_end=False):
    """(name, emissions, transitions) per state: ^ first; state i goes to the
    states of mask[i] in index order and, for i in end_from, to $"""
    n = len(names)
    out = [(START, [""], [names[j] for j in start_to] + ([END] if start_end else []))]
    for i in range(n):
        tr = [names[j] for j in np.flatnonzero(mask[i])] + ([END] if i in end_from else [])
        assert tr and emis[i], names[i]
        out.append((names[i], list(emis[i]), tr))
    return out


def _ring_mask(rng, n, density, skip=()):
    """a random mask of that density plus the ring i -> i + 1 over the states not in skip (no edge into those)"""
    mask = rng.random((n, n)) < density
    ring = [i for i in range(n) if i not in skip]
    for a, b in zip(ring, ring[1:] + ring[:1]):
        mask[a, b] = True
    mask[:, list(skip)] = False
    return mask


def _emissions(rng, n, letters, k):
    return ["".join(sorted(rng.choice(list(letters), size=k, replace=False))) for _ in range(n)]


class _Walker:
    """the automaton as sets, for choosing corpora: structure only"""

    def __init__(self, states):
        self.em = {nm: set(e) for nm, e, _ in states}
        self.tr = {nm: list(t) for nm, _, t in states}

    def paths(self, s):
        """(accepting paths, the bytes after which a state was still alive)"""
        front, alive = {START: 1}, 0
        for c in s:
            nxt = {}
            for u, k in front.items():
                for v in self.tr[u]:
                    if v != END and c in self.em[v]:
                        nxt[v] = nxt.get(v, 0) + k
            front = nxt
            if not front:
                break
            alive += 1
        return sum(k for u, k in front.items() if END in self.tr[u]) if alive == len(s) else 0, alive

    def walk(self, rng, length, tries=10000):
        """a random accepted string of that length (a walk that can end where it stands)"""
        for _ in range(tries):
            u, out = START, []
            for _ in range(length):
                nxt = [v for v in self.tr[u] if v != END]
                if not nxt:
                    break
                u = nxt[rng.integers(len(nxt))]
                out.append(sorted(self.em[u])[rng.integers(len(self.em[u]))])
            if len(out) == length and END in self.tr[u]:
                return "".join(out)
        raise AssertionError("no accepted walk of that length")


def _pack(strings):
    raw = [s.encode("latin-1") for s in strings]
    sym = np.frombuffer(b"".join(raw), dtype=np.uint8).copy()
    off = np.concatenate([[0], np.cumsum([len(s) for s in raw])]).astype(np.int64)
    wt = 1.0 + np.sqrt(np.arange(len(raw)) + 2.0)
    return sym, off, wt / wt.sum()


def _gadget(name, states, strings, R, T, draw=None, **notes):
    sym, off, p = _pack(strings)
    n = len(states) - 1
    notes.update(name=name, states=states, strings=list(strings), n=n, np=-(-n // TILE) * TILE,
                 draw=draw or (sum(map(ord, name)), -1.0, 0.7))
    return Gadget(wfsa_text(states), sym, off, p, R, T, notes)


# -- holes12 ---------------------------------------------------------------------

HOLES = dict(no_start=(5, 6), no_end=(2, 5, 10), only_end=9, unreached=11, one_emission=(3, 7),
             one_transition=(9, 10), density=0.35)


@functools.lru_cache(maxsize=None)
def holes12():
    """12 states, a third of A present; the corpus in the order that puts a
    dead string under a live one in one slot: the longer live strings, the
    dead strings (the shortest of the first 128), then short live strings"""
    rng = np.random.default_rng(1212)
    n, h = 12, HOLES
    mask = _ring_mask(rng, n, 0.38, skip=(h["unreached"],))
    mask[h["only_end"], :] = False
    mask[10, :] = False
    mask[10, 3] = True
    mask[h["unreached"], [0, 4]] = True
    emis = _emissions(rng, n, "abc", 2)
    for i in range(0, n, 2):
        emis[i] = "abc"
    for i in h["no_end"][:2]:
        emis[i] += "d"          # d only where no transition to $ follows: a string ending in d is never accepted
    for i, e in zip(h["one_emission"], "ab"):
        emis[i] = e
    start_to = [i for i in range(n) if i not in h["no_start"] + (h["unreached"],)]
    end_from = set(range(n)) - set(h["no_end"])
    states = _states(_names(n), mask, start_to, end_from, emis, start_end=True)
    wk = _Walker(states)
    seen, one, many, mid, died, unended = set(), [], [], [], [], []
    for _ in range(6000):
        L = int(rng.integers(5, 10))
        s = "".join(rng.choice(list("abcd"), size=L))
        if s in seen:
            continue
        seen.add(s)
        k, _ = wk.paths(s)
        if k == 1:
            one.append(s)
        elif k >= 1000:
            many.append(s)
        elif k > 1:
            mid.append(s)
    for t in itertools.product("abcd", repeat=4):   # the dead strings: the shortest of the first 128
        s = "".join(t)
        k, alive = wk.paths(s)
        if k == 0 and alive == 3:
            died.append(s)          # alive for three bytes, then no edge
        elif k == 0 and alive == 4:
            unended.append(s)       # alive to its last byte, no state there goes to $
    assert len(one) >= 6 and len(many) >= 6 and len(died) >= 4 and len(unended) >= 3 and len(mid) >= 120, \
        [len(x) for x in (one, many, died, unended, mid)]
    live_long = one[:6] + many[:6]
    live_long += [s for s in mid if len(s) == 9][:2]
    dead = died[:4] + unended[:3] + [live_long[0][:2] + "z" + live_long[0][2]]   # a byte nobody emits, in the middle
    live_long += mid[:128 - len(dead) - len(live_long)]
    short = []
    for L in (1, 2, 3):
        cand = sorted({wk.walk(rng, L) for _ in range(40)})
        short += cand[:10]
    strings = live_long + dead + [""] + short
    dead_idx = list(range(len(live_long), len(live_long) + len(dead)))
    return _gadget("holes12", states, strings, 128, 9, dead=dead_idx, empty=len(live_long) + len(dead),
                   one_path=list(range(6)), many_paths=list(range(6, 12)))


# -- the tile edges ----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _device_order(n):
    """names such that names[k] is the state the library numbers k (^ and $
    left out), for an automaton whose text lists `hub` first: a state nothing
    reaches that goes to every other state in this order, so that the states
    enter the library's table in an order the edges do not depend on.
    Returns (names in device order, the hub's index)"""
    import wfsa_amd as W
    special = {0, TILE - 2, TILE - 1, TILE, n - 1}
    for hub in ("hub", "hub1", "hub2", "hub3", "hub4", "hub5"):   # (a name whose place is none of the special ones)
        names = _names(n - 1) + [hub]
        skeleton = [(hub, ["a", "b"], names[:-1]), (START, [""], [names[0]])] + [(nm, ["a", "b"], [names[0], END]) for nm in names[:-1]]
        fsa = W.Fsa.read_text(wfsa_text(skeleton))
        order = [nm for nm in fsa.state_names() if nm not in (START, END)]
        assert sorted(order) == sorted(names)
        if order.index(hub) not in special:
            return order, order.index(hub)
    raise AssertionError("every hub name tried lands on a special index")


def _edge(n):
    """n states; in the library's numbering: ^ goes to state 0 and the last
    state only, only the last state of the first tile (126 at n = 127, else
    127) and state 128 go to $.  One state (hub) is reached by nothing"""
    rng = np.random.default_rng(1000 + n)
    order, hub = _device_order(n)
    start_to = [0, n - 1]
    end_from = {min(n - 1, TILE - 1)} | ({TILE} if n > TILE else set())
    assert hub not in start_to and hub not in end_from
    mask = _ring_mask(rng, n, 0.3, skip=(hub,))
    mask[hub, :] = True
    mask[hub, hub] = False
    emis = _emissions(rng, n, "abcd", 2)
    body = _states(order, mask, start_to, end_from, emis)
    # the hub's row first, its transitions in the skeleton's order; then ^; then the states in the skeleton's order
    by_name = {nm: st for nm, *st in body}
    first = (order[hub], by_name[order[hub]][0], _names(n - 1))
    states = [body[0]] + [(nm, *by_name[nm]) for nm in order]
    text_states = [first, body[0]] + [(nm, *by_name[nm]) for nm in _names(n - 1)]
    wk = _Walker(states)
    strings, seen = [], set()
    for L in (1, 2, 2, 3, 3, 3) + (4, 5, 6, 7, 8) * 8:
        for _ in range(400):
            s = "".join(rng.choice(list("abcd"), size=L))
            if s not in seen and wk.paths(s)[0] > 0:
                strings.append(s)
                seen.add(s)
                break
    strings = strings[:40]
    g = _gadget(f"edge{n}", states, strings, 128, 8, hub=hub, start_to=start_to, end_from=sorted(end_from))
    return g._replace(text=wfsa_text(text_states))


def edge127():
    return _edge(127)


def edge128():
    return _edge(128)


def edge129():
    return _edge(129)


# -- row and column tiles ------------------------------------------------------------

def _random_model(rng, n, density, letters, k, start_frac=0.5, end_frac=0.5):
    mask = _ring_mask(rng, n, density)
    start_to = sorted(rng.choice(n, size=max(2, int(n * start_frac)), replace=False))
    end_from = set(rng.choice(n, size=max(2, int(n * end_frac)), replace=False).tolist())
    return _states(_names(n), mask, start_to, end_from, _emissions(rng, n, letters, k))


@functools.lru_cache(maxsize=None)
def tiles384():
    """257 states: np = 384, three column tiles, split-K halves of 192; 300
    strings of length 3: three row tiles, 9 and 18 blocks"""
    rng = np.random.default_rng(384)
    states = _random_model(rng, 257, 0.3, "abcd", 2)
    wk = _Walker(states)
    return _gadget("tiles384", states, [wk.walk(rng, 3) for _ in range(300)], 384, 3)


@functools.lru_cache(maxsize=None)
def rows256():
    """129 strings of length 4: the second row tile holds one string"""
    rng = np.random.default_rng(256)
    states = _random_model(rng, 8, 0.5, "abcd", 2)
    wk = _Walker(states)
    return _gadget("rows256", states, [wk.walk(rng, 4) for _ in range(129)], 256, 4)


@functools.lru_cache(maxsize=None)
def xcd512():
    """130 states (np = 256), 400 strings of length 2: four row tiles by two
    column tiles, 8 blocks (16 with split K): the XCD renumbering taken"""
    rng = np.random.default_rng(512)
    states = _random_model(rng, 130, 0.3, "abcd", 2)
    wk = _Walker(states)
    return _gadget("xcd512", states, [wk.walk(rng, 2) for _ in range(400)], 512, 2)


@functools.lru_cache(maxsize=None)
def single():
    rng = np.random.default_rng(1)
    states = _random_model(rng, 8, 0.5, "abcd", 2)
    return _gadget("single", states, [_Walker(states).walk(rng, 5)], 128, 5)


@functools.lru_cache(maxsize=None)
def t1():
    """48 symbols, every accepted string of length 1: no GEMM, no interior transition used"""
    rng = np.random.default_rng(11)
    letters = ALPHABET[:48]
    states = _random_model(rng, 8, 0.5, letters, 8, start_frac=0.75, end_frac=0.75)
    # every letter has a state: state i also emits letters i, i + 8, ...
    states = [states[0]] + [(nm, sorted(set(em) | set(letters[i::8])), tr) for i, (nm, em, tr) in enumerate(states[1:])]
    wk = _Walker(states)
    strings = [c for c in letters if wk.paths(c)[0] > 0]
    assert 30 <= len(strings) <= 128
    return _gadget("t1", states, strings, 128, 1)


SEAMS_RUN = 11   # length-1 strings back to back in one slot: T = 12 holds no more than 12


@functools.lru_cache(maxsize=None)
def seams():
    """one string of length 12, 20 of length 3, 20 of length 2 and 1280 of
    length 1: 128 slots of 12 steps, 87 of them filled with length-1 strings
    only -- start and end flag on one row, row after row"""
    rng = np.random.default_rng(12)
    letters = ALPHABET[:20]
    states = _random_model(rng, 8, 0.6, letters, 8, start_frac=0.75, end_frac=0.75)
    wk = _Walker(states)
    ones = [c for c in letters if wk.paths(c)[0] > 0]
    assert len(ones) >= 10
    strings = [wk.walk(rng, 12)] + [wk.walk(rng, 3) for _ in range(20)] + [wk.walk(rng, 2) for _ in range(20)]
    strings += [ones[int(rng.integers(len(ones)))] for _ in range(1280)]
    return _gadget("seams", states, strings, 128, 12)


# -- wide vocabularies -----------------------------------------------------------------

def _vocab(v):
    """6 states, fully connected, v distinct bytes, each emitted by two
    states; string i is symbols i, i + 1, i + 2 (cyclic): every symbol at a
    start, an interior and an end position"""
    rng = np.random.default_rng(v)
    n, letters = 6, ALPHABET[:v]
    emis = [[] for _ in range(n)]
    for k, c in enumerate(letters):
        a = k % n
        b = (a + 1 + int(rng.integers(n - 1))) % n
        emis[a].append(c)
        emis[b].append(c)
    states = _states(_names(n), np.ones((n, n), bool), list(range(n)), set(range(n)), emis)
    strings = [letters[i] + letters[(i + 1) % v] + letters[(i + 2) % v] for i in range(v)]
    R = slot_shape([3] * v, TILE)[0]
    assert R == (128 if v <= 128 else 256)
    return _gadget(f"vocab{v}", states, strings, R, 3, vocab=v)


def vocab65():
    return _vocab(65)


def vocab94():
    return _vocab(94)


def vocab130():
    """a third window: bytes from 0xa1 on (the text reader takes them from bytes)"""
    return _vocab(130)


# -- precision -------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def long300():
    """3 states, weights N(-20, 1), 4 strings of length 300: log q near -12000"""
    rng = np.random.default_rng(300)
    n = 3
    states = _states(_names(n), np.ones((n, n), bool), [0, 1, 2], {0, 1, 2}, ["ab", "bc", "ac"])
    wk = _Walker(states)
    return _gadget("long300", states, [wk.walk(rng, 300) for _ in range(4)], 128, 300, draw=(300, -20.0, 1.0))


PEAKED_GAP = 40.0


@functools.lru_cache(maxsize=None)
def peaked():
    """s0 -> s1 -> s3 and s0 -> s2 -> s3 emit the same bytes; the weights of
    s0's two transitions differ by 40: the route over s2 has posterior e^-40 = 4e-18"""
    rng = np.random.default_rng(40)
    states = [(START, [""], ["s0", "s3"]), ("s0", ["a", "b"], ["s1", "s2"]), ("s1", ["a", "b"], ["s3", END]),
              ("s2", ["a", "b"], ["s3", END]), ("s3", ["a", "b"], ["s0", END])]
    wk = _Walker(states)
    strings = ["aba", "ab"] + [wk.walk(rng, int(L)) for L in rng.integers(3, 9, size=8)]
    fixed = {("s0", "T", "s1"): -0.5, ("s0", "T", "s2"): -0.5 - PEAKED_GAP, ("s1", "T", "s3"): -0.7, ("s1", "T", END): -0.7,
             ("s2", "T", "s3"): -0.7, ("s2", "T", END): -0.7}
    return _gadget("peaked", states, strings, 128, max(len(s) for s in strings), set=fixed,
                   rare=[("s0", "T", "s2"), ("s2", "T", "s3"), ("s2", "T", END)])


GADGETS = {f.__name__: f for f in (holes12, edge127, edge128, edge129, tiles384, rows256, xcd512, single, t1, seams,
                                   vocab65, vocab94, vocab130, long300, peaked)}
ENUM_GADGETS = ("holes12", "single", "t1", "seams", "rows256", "peaked")


# -- the automatic choice ------------------------------------------------------------------

def choice_model(n, per_state, drop=0):
    """n states, each going to the next per_state states (cyclic) and to $,
    the last `drop` transitions of state 0 left out; n * per_state - drop interior transitions"""
    names = _names(n)
    states = [(START, [""], [names[0], names[1]])]
    for i in range(n):
        k = per_state - (drop if i == 0 else 0)
        states.append((names[i], ["a", "b"], [names[(i + 1 + j) % n] for j in range(k)] + [END]))
    return wfsa_text(states)


def two_byte_model():
    return wfsa_text([(START, [""], ["s0", "s1"]), ("s0", ["a", "bc"], ["s0", "s1", END]), ("s1", ["a", "b"], ["s0", "s1", END])])


def epsilon_model():
    return wfsa_text([(START, [""], ["s0", "s1"]), ("s0", ["a", ""], ["s1", END]), ("s1", ["a", "b"], ["s0", "s1", END])])
