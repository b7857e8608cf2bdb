"""The hand-built dense-path cases (dense_gadgets.py) checked without a
device: the long-double reference against the oracle -- its enumerated paths
for the small gadgets, its trellis for the larger ones -- at log q rel 1e-13,
gradient rel 1e-12 (absolute floor 1e-18) and smallest relative path
probability rel 1e-12; the row slots the gadgets promise (slot_shape); the
holes, single-member groups, windows and dead strings they promise; and five
mistakes a dense kernel could make, injected one at a time into a float64
restatement, each of which some gadget tells from the reference at the GPU
tests' own bounds (test_gpu_dense_gadgets.py)."""
import functools

import numpy as np
import pytest

import dense_gadgets as G

LD = np.longdouble
LOGQ_REL, GRAD_REL, GRAD_FLOOR, RMIN_REL = 1e-13, 1e-12, 1e-18, 1e-12


@functools.lru_cache(maxsize=None)
def _case(name):
    """(gadget, fsa, parameter names, weights, reference over the recognized strings, their indices)"""
    import wfsa_amd as W
    g = G.GADGETS[name]()
    fsa = W.Fsa.read_text(g.text.encode("latin-1"))
    names = fsa.param_names()
    w = G.weights(g, names)
    whole = G.reference(fsa, w, g.sym, g.off, g.p)
    keep = np.flatnonzero([k > 0 for k in whole.paths])
    sym, off, p = _subset(g, keep)
    ref = G.reference(fsa, w, sym, off, p) if len(keep) < len(g.p) else whole
    for a in (ref.logq, ref.grad, ref.rmin):
        a.setflags(write=False)
    return g, fsa, names, w, whole, ref, keep


def _subset(g, keep):
    strings = [bytes(g.sym[g.off[i]:g.off[i + 1]]) for i in keep]
    sym = np.frombuffer(b"".join(strings), dtype=np.uint8).copy()
    off = np.concatenate([[0], np.cumsum([len(s) for s in strings])]).astype(np.int64)
    return sym, off, g.p[keep] / g.p[keep].sum()   # (the oracle normalises p over the strings it is given)


def _tables(name):
    from dense_decode_reference import Tables
    g, fsa, _, w, *_ = _case(name)
    return g, Tables(fsa, w)


# -- the reference against the oracle ------------------------------------------------

@pytest.mark.parametrize("name", G.ENUM_GADGETS)
def test_reference_equals_path_enumeration(name):
    """recognition and path counts exactly; log q, the gradient and the
    smallest relative path probability from a long-double sum over the
    oracle's enumerated paths"""
    from oracle import ENUM, Oracle
    g, fsa, names, w, whole, ref, keep = _case(name)
    text = g.text.encode("latin-1")
    o = Oracle.from_arrays(text, g.sym, g.off, g.p, mode=ENUM, max_paths=10_000_000)
    assert [int(k) for k in o.path_counts()] == whole.paths
    sym, off, p = _subset(g, keep)
    o = Oracle.from_arrays(text, sym, off, p, mode=ENUM, max_paths=10_000_000)
    full = o.full_param_names()
    assert sorted(full) == sorted(names)
    # the oracle's path matrices leave out a used parameter that is the only used one of its group (the learner
    # fixes it at 0): the comparison runs at the gadget's weights with 0 on those (the trellis test covers them)
    state = dict(zip(full, o.trimmed_index()))
    fixed = [nm for nm in names if state[nm] == -1]
    w0 = np.array([0.0 if state[nm] == -1 else x for nm, x in zip(names, w)])
    ref = G.reference(fsa, w0, sym, off, p) if fixed else ref
    by_name = dict(zip(names, w0))
    trimmed = o.param_names()
    assert [nm for nm in names if state[nm] >= 0] == [nm for nm in names if nm in set(trimmed)]
    wt = np.array([by_name[nm] for nm in trimmed], dtype=LD)
    prow, pcol, pdata, mrow = o.paths()
    assert len(mrow) == len(keep) + 1 and [int(b - a) for a, b in zip(mrow, mrow[1:])] == [whole.paths[i] for i in keep]
    lw = np.array([np.sum(pdata[prow[l]:prow[l + 1]].astype(LD) * wt[pcol[prow[l]:prow[l + 1]]]) for l in range(len(prow) - 1)],
                  dtype=LD)
    logq, rmin, grad_t = np.zeros(len(keep), LD), np.zeros(len(keep), LD), np.zeros(len(trimmed), LD)
    for s in range(len(keep)):
        a, b = mrow[s], mrow[s + 1]
        top = lw[a:b].max()
        logq[s] = top + np.log(np.sum(np.exp(lw[a:b] - top)))
        post = np.exp(lw[a:b] - logq[s])
        rmin[s] = post.min()
        for l, r in zip(range(a, b), post):
            np.add.at(grad_t, pcol[prow[l]:prow[l + 1]], -LD(p[s]) * r * pdata[prow[l]:prow[l + 1]])
    grad = dict.fromkeys(names, LD(0))
    grad.update(zip(trimmed, grad_t))
    free = np.array([state[nm] != -1 for nm in names])
    assert G.close(ref.logq, logq, LOGQ_REL)
    assert G.close(ref.grad[free], np.array([grad[nm] for nm in names])[free], GRAD_REL, GRAD_FLOOR)
    assert (ref.grad[~free] < 0).all() and (ref.grad[[state[nm] == -2 for nm in names]] == 0).all()
    assert G.close(ref.rmin, rmin, RMIN_REL)
    assert G.close(ref.ll, np.sum(p.astype(LD) * logq), LOGQ_REL)
    assert [bool(u) for u in ref.used] == [state[nm] != -2 for nm in names]


@pytest.mark.parametrize("name", G.GADGETS)
def test_reference_equals_trellis_oracle(name):
    """every gadget at its own weights, over its recognized strings"""
    from oracle import Oracle, TRELLIS
    g, fsa, names, w, whole, ref, keep = _case(name)
    assert len(keep) == len(g.p) or name == "holes12"   # (every string of the other gadgets is accepted)
    sym, off, p = _subset(g, keep)
    o = Oracle.from_arrays(g.text.encode("latin-1"), sym, off, p, mode=TRELLIS)
    by_name = dict(zip(names, w))
    full = o.full_param_names()
    assert sorted(full) == sorted(names)
    # long300: the oracle's trellis is unscaled and underflows near e^-12000.  Every path of a string of length L
    # there takes one start, L emission, L - 1 interior and one end parameter, so c added to every weight adds
    # (2 L + 1) c to log q and leaves the posteriors alone: the oracle runs at w + 20
    shift = 20.0 if name == "long300" else 0.0
    ll, logq, grad = o.trellis_eval(np.array([by_name[nm] + shift for nm in full]))
    if shift:
        from dense_decode_reference import Tables
        tab = Tables(fsa, w)
        assert min(t.min() for t in (tab.pA, tab.p0, tab.pend)) >= 0 and set(tab.pE[tab.pE != -2]) == set(tab.pE[tab.pE >= 0])
        per = (2 * np.diff(off) + 1) * shift
        logq = logq.astype(LD) - per
        ll = LD(ll) - np.sum(p.astype(LD) * per)
    grad = dict(zip(full, grad))
    assert G.close(ref.logq, logq, LOGQ_REL)
    assert G.close(ref.ll, ll, LOGQ_REL)
    assert G.close(ref.grad, [grad[nm] for nm in names], GRAD_REL, GRAD_FLOOR)
    if float(g.notes["n"]) ** int(np.diff(g.off).max()) < 2.0 ** 62:
        assert [int(k) for k in o.path_counts()] == [whole.paths[i] for i in keep]


# -- the row slots -----------------------------------------------------------------------

TABLE = {"holes12": (128, 9), "edge127": (128, 8), "edge128": (128, 8), "edge129": (128, 8), "tiles384": (384, 3),
         "rows256": (256, 4), "xcd512": (512, 2), "single": (128, 5), "t1": (128, 1), "seams": (128, 12),
         "vocab65": (128, 3), "vocab94": (128, 3), "vocab130": (256, 3), "long300": (128, 300)}
NP = {"holes12": 128, "edge127": 128, "edge128": 128, "edge129": 256, "tiles384": 384, "xcd512": 256}


@pytest.mark.parametrize("name", G.GADGETS)
def test_slot_shape_gives_the_promised_rows_and_steps(name):
    g = G.GADGETS[name]()
    lengths = np.diff(g.off)
    R, T, slots = G.slot_shape(lengths, g.notes["np"])
    assert (R, T) == (g.R, g.T)
    if name in TABLE:
        assert (g.R, g.T) == TABLE[name]
    assert g.notes["np"] == NP.get(name, 128)
    assert (R // 128) * (g.notes["np"] // 128) <= 16            # the rule's block count: it does not see the CU count
    placed = sorted(i for s in slots for i in s)
    assert placed == [i for i, n in enumerate(lengths) if n > 0]
    assert max(sum(lengths[i] for i in s) for s in slots) == T


def test_slot_shape_rule():
    """the rule on shapes worked out by hand"""
    assert G.slot_shape([4] * 129, 128)[:2] == (256, 4)        # 128: t = 5, cost 4; 256: t = 4, cost 3
    assert G.slot_shape([4] * 128, 128)[:2] == (128, 4)
    assert G.slot_shape([3] * 300, 384)[:2] == (384, 3)        # costs 7, 3, 2
    assert G.slot_shape([2] * 400, 256)[:2] == (512, 2)        # costs 6, 3, 2, 1
    assert G.slot_shape([12] + [1] * 300, 128)[:2] == (128, 12)   # costs 11, 11, 11: the first
    assert G.slot_shape([0, 0], 128)[:2] == (128, 1)
    R, T, slots = G.slot_shape([5, 1, 1, 1, 0, 3], 128)
    assert (R, T) == (128, 5) and slots[:5] == [[0], [5], [1], [2], [3]]
    # with 4 CUs the rounds count: 2 row tiles by 3 column tiles are 2 rounds (cost 6), one row tile 1 round (cost 4)
    assert G.slot_shape([4] * 129, 384, n_cu=4)[:2] == (128, 8)


def test_holes12_and_seams_slots():
    g = G.holes12()
    lengths = np.diff(g.off)
    _, _, slots = G.slot_shape(lengths, 128)
    dead = set(g.notes["dead"])
    pairs = [(s[k], s[k + 1]) for s in slots for k in range(len(s) - 1) if s[k] in dead and s[k + 1] not in dead]
    assert len(pairs) >= 5
    whole = _case("holes12")[4]
    # a string that died mid-way (no state alive), and one alive to its end without a way to $, each under a live string
    died = {i for i in dead if _alive(g, i) < lengths[i]}
    assert any(a in died for a, _ in pairs) and any(a not in died for a, _ in pairs)
    assert all(whole.paths[a] == 0 and whole.paths[b] > 0 for a, b in pairs)
    g = G.seams()
    lengths = np.diff(g.off)
    _, _, slots = G.slot_shape(lengths, 128)
    runs = [sum(1 for i in s if lengths[i] == 1) for s in slots if all(lengths[i] == 1 for i in s)]
    # a slot holds T = 12 symbols: 11 length-1 strings back to back is what 1280 of them over 127 slots give
    assert max(runs) >= G.SEAMS_RUN and sum(r >= G.SEAMS_RUN for r in runs) >= 20
    assert max(len(s) for s in slots) <= 12 and sum(len(s) > 1 for s in slots) == 127


def _alive(g, i):
    return G._Walker(g.notes["states"]).paths(g.notes["strings"][i])[1]


# -- what the gadgets promise ----------------------------------------------------------------

def test_holes12_preconditions():
    g, tab = _tables("holes12")
    h, whole = G.HOLES, _case("holes12")[4]
    present = tab.pA != -2
    assert tab.n == 12 and 0.25 <= present.mean() <= 0.40   # 42 of 144: the rows of the two single-transition states are all but empty
    assert (tab.p0 == -2).sum() == 3 and (tab.pend == -2).sum() == 3    # (the unreached state has no ^ -> T either)
    assert tab.pse >= 0
    assert ((~present).all(axis=1) & (tab.pend == -1)).sum() == 1        # only way out: $, a single-member group
    assert (~present).all(axis=0).sum() == 1                             # nothing reaches it
    unreached = int(np.flatnonzero((~present).all(axis=0))[0])
    assert tab.p0[unreached] == -2 and present[unreached].any()
    assert ((tab.pE == -1).sum(axis=1) == 1).sum() == 2 == len(h["one_emission"])
    one_tr = (present.sum(axis=1) + (tab.pend != -2)) == 1
    assert one_tr.sum() == 2 and (tab.pA == -1).sum() == 1 and (tab.pend == -1).sum() == 1
    lengths = np.diff(g.off)
    notes = g.notes
    assert [i for i, k in enumerate(whole.paths) if k == 0] == notes["dead"] and len(notes["dead"]) == 8
    assert lengths[notes["empty"]] == 0 and whole.paths[notes["empty"]] == 1 and (lengths == 0).sum() == 1
    assert all(whole.paths[i] == 1 for i in notes["one_path"]) and all(whole.paths[i] >= 1000 for i in notes["many_paths"])
    alive = [_alive(g, i) for i in notes["dead"]]
    assert sum(a >= 3 and a < lengths[i] for a, i in zip(alive, notes["dead"])) >= 4     # alive for three bytes, then dead
    assert sum(a == lengths[i] for a, i in zip(alive, notes["dead"])) == 3               # alive to the end, no T -> $ there
    z = notes["strings"][notes["dead"][-1]]
    assert z[2] == "z" and len(z) == 4 and (tab.pE[:, ord("z")] == -2).all()
    assert (lengths == 1).sum() >= 3 and (lengths > 0).sum() > 128
    assert (~whole.used).sum() >= 2          # parameters no string uses: their gradient is exactly 0
    assert np.array_equal(whole.grad == 0, ~whole.used)


@pytest.mark.parametrize("n", [127, 128, 129])
def test_edge_preconditions(n):
    """in the library's own numbering: ^ -> state 0 and the last state only,
    $ only from the last state of the first tile and from state 128"""
    g, tab = _tables(f"edge{n}")
    assert tab.n == n
    assert list(np.flatnonzero(tab.p0 != -2)) == [0, n - 1] == g.notes["start_to"]
    assert list(np.flatnonzero(tab.pend != -2)) == {127: [126], 128: [127], 129: [127, 128]}[n] == g.notes["end_from"]
    present = tab.pA != -2
    hub = g.notes["hub"]
    assert list(np.flatnonzero(~present.any(axis=0))) == [hub] and present[hub].sum() == n - 1
    rest = np.delete(np.delete(present, hub, axis=0), hub, axis=1)
    assert 0.27 <= rest.mean() <= 0.36
    ring = [i for i in range(n) if i != hub]
    assert all(present[a, b] for a, b in zip(ring, ring[1:] + ring[:1]))
    lengths = np.diff(g.off)
    assert len(lengths) <= 40 and lengths.max() == 8 and lengths.min() <= 2
    whole = _case(f"edge{n}")[4]
    assert all(k > 0 for k in whole.paths)
    if n == 129:   # the state alone in the second tile carries weight: start, end and interior edges through it are used
        used = {int(c) for c in np.flatnonzero(whole.used)}
        assert tab.p0[128] in used and tab.pend[128] in used
        assert used & set(tab.pA[128][tab.pA[128] >= 0]) and used & set(tab.pA[:, 128][tab.pA[:, 128] >= 0])


def test_other_preconditions():
    g, tab = _tables("tiles384")
    assert tab.n == 257 and len(g.p) == 300 and set(np.diff(g.off)) == {3}
    g, tab = _tables("rows256")
    assert tab.n == 8 and len(g.p) == 129 and set(np.diff(g.off)) == {4}
    g, tab = _tables("xcd512")
    assert tab.n == 130 and len(g.p) == 400 and set(np.diff(g.off)) == {2}
    # fused: 4 x 2 blocks, split: 16 -- multiples of 8, the XCD renumbering taken; tiles384: 9 and 18, not taken
    assert (512 // 128) * (256 // 128) % 8 == 0 and (384 // 128) * (384 // 128) % 8 != 0 and 2 * 9 % 8 != 0
    g, tab = _tables("single")
    assert len(g.p) == 1 and np.diff(g.off)[0] == 5
    g, tab = _tables("t1")
    whole = _case("t1")[4]
    strings = g.notes["strings"]
    assert (tab.pE != -2).any(axis=0).sum() >= 40 and len(set(strings)) == len(strings) <= 128 and set(map(len, strings)) == {1}
    assert (whole.grad[tab.pA[tab.pA >= 0]] == 0).all() and (tab.pA >= 0).sum() > 20    # no interior transition is used
    g, tab = _tables("peaked")
    names, whole = _case("peaked")[2], _case("peaked")[4]
    rare = [names.index(nm) for nm in g.notes["rare"]]
    assert all(0 < -whole.grad[j] < 1e-15 for j in rare) and (-whole.grad).max() > 0.5
    by_name = dict(zip(names, _case("peaked")[3]))
    assert by_name[("s0", "T", "s1")] - by_name[("s0", "T", "s2")] == G.PEAKED_GAP
    g, tab = _tables("long300")
    assert set(np.diff(g.off)) == {300} and -12500 < _case("long300")[4].ll < -11500


@pytest.mark.parametrize("v", [65, 94, 130])
def test_vocab_preconditions(v):
    """the device numbers the used bytes in byte order: the windows are
    symbols [0, 64), [64, 128), [128, ...); every symbol stands at a start,
    an interior and an end position of some string"""
    g, tab = _tables(f"vocab{v}")
    used = np.flatnonzero((tab.pE != -2).any(axis=0))
    assert len(used) == v == g.notes["vocab"]
    windows = [len(used[k:k + G.RED_WINDOW]) for k in range(0, v, G.RED_WINDOW)]
    assert windows == {65: [64, 1], 94: [64, 30], 130: [64, 64, 2]}[v]
    if v == 130:
        assert (used >= 0x80).sum() == 36
    strings = [bytes(g.sym[g.off[i]:g.off[i + 1]]) for i in range(len(g.p))]
    for pos in (0, 1, 2):
        assert sorted(s[pos] for s in strings) == list(used)
    whole = _case(f"vocab{v}")[4]
    em = tab.pE[tab.pE >= 0]
    assert (whole.grad[em] < 0).all() and whole.used.all()


def test_automatic_choice_models():
    """the models of the GPU test of dense_model_build's admission rule"""
    import wfsa_amd as W

    def interior(text):
        from dense_decode_reference import Tables
        fsa = W.Fsa.read_text(text)
        tab = Tables(fsa, np.zeros(fsa.counts()["parameters"]))
        return tab.n, int((tab.pA != -2).sum())
    assert interior(G.choice_model(64, 16)) == (64, 1024)
    assert interior(G.choice_model(64, 16, drop=1)) == (64, 1023)
    assert interior(G.choice_model(63, 63)) == (63, 63 * 63)
    assert W.Fsa.read_text(G.two_byte_model()).counts()["states"] == 4
    assert W.Fsa.read_text(G.epsilon_model()).counts()["states"] == 4


# -- float64, and the faults it must not hide ------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _restated(name, fault):
    g, fsa, names, w, whole, ref, keep = _case(name)
    return G.restate(fsa, w, g.sym, g.off, g.p, fault=fault)


def _agrees(name, fault):
    """restate(fault) against the reference at the GPU tests' bounds of that gadget"""
    g, fsa, names, w, whole, ref, keep = _case(name)
    logq, ll, grad, rmin = _restated(name, fault)
    f64 = _f64_distance(name) if fault else (0.0, 0.0, 0.0)
    lq_rel, g_rel, r_rel = G.bounds(name, f64)
    live = np.isfinite(whole.logq) & (np.diff(g.off) > 0)
    return (G.close(logq, whole.logq, lq_rel) and G.close(grad, whole.grad, g_rel, G.GRAD_ATOL)
            and G.close(rmin[live], whole.rmin[live], r_rel))


def _f64_distance(name):
    g, fsa, names, w, whole, ref, keep = _case(name)
    logq, ll, grad, rmin = _restated(name, None)
    live = np.isfinite(whole.logq) & (np.diff(g.off) > 0)
    return (G.distance(logq, whole.logq), G.distance(grad, whole.grad, G.GRAD_ATOL), G.distance(rmin[live], whole.rmin[live]))


@pytest.mark.parametrize("name", G.GADGETS)
def test_float64_meets_the_bounds(name):
    """the device's number format can meet every bound: the float64
    restatement is 16 times inside it (holes12's dead strings at -inf, p > 0
    on them: LL is -inf on both sides)"""
    d = _f64_distance(name)
    print(f"dense_gadgets f64 distance | {name} | logq {d[0]:.3e} grad {d[1]:.3e} rmin {d[2]:.3e}")
    for dist, bound in zip(d, G.bounds(name, d)):
        assert G.ORDER_FACTOR * dist <= bound
    if name not in G.LOOSENED:
        assert G.bounds(name, d) == (G.LOGQ_REL, G.GRAD_REL, G.RMIN_REL)


@pytest.mark.parametrize("fault,where", [
    ("last_tile", ("edge129",)),
    ("start_as_continuation", ("holes12", "seams")),
    ("symbols_from_64", ("vocab65", "vocab94", "vocab130")),
    ("no_start_end_edge", ("holes12",)),
    ("dead_scale_leaks", ("holes12",)),
])
def test_injected_faults_are_seen(fault, where):
    """one mistake at a time: the gadgets built for it tell it from the
    reference, and no gadget that cannot reach it is disturbed"""
    assert fault in G.FAULTS
    for name in where:
        assert not _agrees(name, fault), name
    for name in ("single", "t1", "rows256"):
        assert _agrees(name, fault), name
