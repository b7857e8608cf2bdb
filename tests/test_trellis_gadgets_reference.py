"""The hand-built trellis cases (trellis_gadgets.py) checked without a device:
every case is what it claims (destination, in-edge and end-edge counts at the
lane-round seams, path counts, which ties exist), the id list in path order
names every path, the reference's enumeration is the ENUM oracle's (path counts
per string and the multiset of count rows with their weights), its orders,
posteriors, MEA decode and sampler replay agree with what can be stated by hand
or is derived elsewhere in the suite, and for the committed seed no sample of
any case is undecidable (test_gpu_trellis_gadgets.py compares every sample)."""
import collections
import math

import numpy as np
import pytest

import marginal_reference as MR
import trellis_gadgets as G
from decode_cases import _tol
from test_gpu_byte_marginals import FIXTURE_A_WEIGHTS


@pytest.fixture(scope="module", autouse=True)
def _drop_caches():
    yield
    G.clear_caches()


def _in_counts(wd, byte):
    return [len(v) for v in wd.ins[ord(byte)]]


def _names(model, l_ids):
    return [model.names[j] for j in l_ids]


# -- each case is what it claims ------------------------------------------------------------------

@pytest.mark.parametrize("w", G.SEAMS)
def test_seam_shape_and_orders(w):
    c = G.seam(w)
    m, wd = c.model, c.model.wide
    assert len(wd.slots[ord("a")]) == w and set(_in_counts(wd, "a")) == {1}
    assert len(wd.slots[ord("x")]) == 1 and _in_counts(wd, "x") == [w + 1]   # H: from ^ and from every a-state
    assert len(m.names) == 3 * w + 1
    slots = [wd.nodes[n] for n in wd.slots[ord("a")]]
    assert wd.slots[ord("a")] == sorted(wd.slots[ord("a")])
    for wn in c.weightings:
        assert len(c.ref(wn, b"xa").paths) == w and len(c.ref(wn, b"xaxa").paths) == w * w
    # zero: every weight ties; the order is the slots' on xa and (second visit, first visit) on xaxa
    r = c.ref("zero", b"xa")
    assert {p.lw for p in r.paths} == {0.0}
    assert [_names(m, r.paths[l].ids) for l in r.order] == [[("H", "T", s), (s, "T", G.END)] for s in slots]
    r = c.ref("zero", b"xaxa")
    want = [[("H", "T", s1), (s1, "T", "H"), ("H", "T", s2), (s2, "T", G.END)] for s2 in slots for s1 in slots]
    assert [_names(m, r.paths[l].ids) for l in r.order] == want
    # raised: the slot of index min(64, w - 1) first, then the others in slot order
    up = min(64, w - 1)
    r = c.ref("raised", b"xa")
    assert [r.paths[l].nodes[1] for l in r.order] == [wd.slots[ord("a")][up]] + [n for k, n in enumerate(wd.slots[ord("a")]) if k != up]
    assert r.paths[r.order[0]].lw == 1.0 and r.paths[r.order[1]].lw == 0.0
    # graded: the 16 best of xa are the slots w - 1 .. w - 16, across the round boundary where w > 64
    r = c.ref("graded", b"xa")
    assert [r.paths[l].nodes[1] for l in r.order[:16]] == wd.slots[ord("a")][::-1][:16]
    r = c.ref("graded", b"xaxa")
    assert len({p.lw for p in r.paths}) == 2 * w - 1   # ties: the sums j1 + j2
    r = c.ref("random", b"xaxa")
    assert len({p.lw for p in r.paths}) == w * w       # none


@pytest.mark.parametrize("shape", G.SEAM2)
def test_seam2_shape(shape):
    w0, w1, w2 = shape
    wd = G.seam2(*shape).model.wide
    assert _in_counts(wd, "c") == [1] * w0 and _in_counts(wd, "a") == [w0] * w1 and _in_counts(wd, "b") == [w1] * w2
    assert _in_counts(wd, "x") == [w2 + 1]
    c = G.seam2(*shape)
    for s in c.distinct:
        assert len(c.ref("zero", s).paths) == w0 * w1 * w2
    r = c.ref("zero", b"xcab")
    # all ties: a b-destination's list is (in-edge, rank) ascending -- w1 sources of w0 ranks each -- and the end takes the slots in order
    first = r.paths[r.order[0]]
    assert list(first.nodes) == \
        [wd.slots[ord("x")][0], wd.slots[ord("c")][0], wd.slots[ord("a")][0], wd.slots[ord("b")][0]]
    assert [r.paths[l].nodes[3] for l in r.order[:w0 * w1 + 1]] == [wd.slots[ord("b")][0]] * (w0 * w1) + [wd.slots[ord("b")][1]]
    assert len({p.lw for p in c.ref("graded", b"xcab").paths}) < w0 * w1 * w2
    assert len({p.lw for p in c.ref("random", b"xcab").paths}) == w0 * w1 * w2


def test_ragged_shapes():
    c = G.ragged()
    wd = c.model.wide
    counts = _in_counts(wd, "b")
    heavy = wd.slots[ord("b")].index(wd.nodes.index(c.heavy))
    assert len(counts) == 65 and sorted(counts) == [1] * 64 + [70] and counts[heavy] == 70 and heavy % G.WAVE != 0
    sources = [src for _, src, _ in wd.ins[ord("b")][heavy]]
    assert len(set(sources)) == 70 and set(sources) == set(wd.slots[ord("a")]) and len(wd.slots[ord("a")]) == 70
    assert len(c.ref("zero", b"xab").paths) == 134 == len(c.ref("zero", b"xabx").paths)
    e = G.ragged_ends()
    wd = e.model.wide
    live = wd.slots[ord("a")]
    ends = [len(wd.ends[n]) for n in live]
    heavy = live.index(wd.nodes.index(e.heavy))
    assert len(live) == 65 and sorted(ends) == [1] * 64 + [70] and ends[heavy] == 70 and heavy % G.WAVE != 0
    assert len(e.ref("zero", b"xa").paths) == 134
    for case in (c, e):
        for s in case.distinct:
            assert len({p.lw for p in case.ref("random", s).paths}) == 134


def test_stale_shape():
    c = G.stale()
    m, wd = c.model, c.model.wide
    node = {n: i for i, n in enumerate(wd.nodes)}
    assert len(c.strings) == 3 * 4096 + 12 > 16 * 256 * 3
    t = wd.slots[ord("c")].index(node["T"])
    assert {src for _, src, _ in wd.ins[ord("c")][t]} == {node["P"], node["Q"], node["Q2"]}
    assert node["P"] not in wd.slots[ord("b")] and wd.slots[ord("a")] == [node["P"]]
    # ac leaves P at position 1, the parity of the row where xabc reads the sources of byte c (position 3)
    assert c.ref("random", b"ac").paths[0].nodes[0] == node["P"] and len(b"xab") % 2 == 1
    w = c.weightings["random"]
    assert w[m.pid[("P", "T", "T")]] == G.STALE_GAP and np.isneginf(w[m.pid[("H", "T", "D")]])
    assert np.abs(np.delete(w, [m.pid[("P", "T", "T")], m.pid[("H", "T", "D")]])).max() < 4.0
    want = {b"ac": 1, b"xabc": 2, b"xac": 1, b"az": 0, b"aa": 0, b"a": 0, b"xaz": 0, b"xd": 1, b"": 0, b"xabcx": 2, b"aba": 0,
            b"abc": 2, b"xab": 1, b"b": 0}
    assert {s: len(c.ref("random", s).paths) for s in c.distinct} == want
    assert c.ref("random", b"xd").finite == [] and c.ref("random", b"xd").posterior["logq"] == -math.inf
    assert ord("z") not in wd.slots   # a byte without a destination
    # a ghost path over the stale P would outweigh both real paths of xabc by about the gap
    r = c.ref("random", b"xabc")
    ghost = w[m.pid[(G.START, "T", "P")]] + w[m.pid[("P", "E", "a")]] + G.STALE_GAP
    assert ghost - max(p.lw for p in r.paths) > 30.0


def test_empty_string_has_one_path_of_one_end_edge():
    for c in (G.empty(), G.empty(alone=True)):
        m = c.model
        for wn, w in c.weightings.items():
            r = c.ref(wn, b"")
            j = m.pid[(G.START, "T", G.END)]
            assert len(r.paths) == 1 and r.paths[0].edges == () and r.paths[0].ids == (j,)
            p = r.posterior
            assert p["logq"] == w[j] == r.sample_logq and p["entropy"] == 0.0 and p["counts"] == {j: 1.0} and p["mass"] == []
            assert r.order == [0] and r.mea([]) == (0, 0.0)
    assert G.empty(alone=True).strings == [b""] and G.empty().strings.count(b"") == 3


def test_composite_features():
    c = G.composite()
    wd = c.model.wide
    assert len(c.strings) == 21 and max(len(c.ref("zero", s).paths) for s in c.distinct) == 960
    pairs = chains = six = xend = 0
    for s in c.distinct:
        r = c.ref("zero", s)
        by_nodes = collections.Counter(p.nodes for p in r.paths)
        pairs += any(n > 1 for n in by_nodes.values())   # parallel edges: the same nodes, other in-edges
        chains += any(n >= wd.n_states for p in r.paths for n in p.nodes)
        six += any(len(r.lw_in[e][1]) == 6 for p in r.paths for e in p.edges)
        xend += any(len(r.lw_end[p.x][1]) >= 3 for p in r.paths)
    assert min(pairs, chains, six, xend) >= 2
    # at zero weights the parallel pair ties and the lower in-edge goes first
    r = c.ref("zero", b"xr")
    same = [l for l in r.order if r.paths[l].nodes == r.paths[r.order[0]].nodes and r.paths[l].x == r.paths[r.order[0]].x]
    assert len(same) == 2 and r.paths[same[0]].edges < r.paths[same[1]].edges
    # the chain nodes' mass goes to their owner: both bytes of pq lie in E2
    p = c.ref("zero", b"xpq").posterior
    assert p["mass"][1] == {c.model.sid["E2"]: 1.0} == p["mass"][2] and p["boundary"] == [1.0, 0.0, 1.0]


def test_few_loop_and_ids65():
    for n in (1, 3):
        c = G.few(n)
        assert all(len(c.ref(wn, b"xa").paths) == n for wn in c.weightings)
    c = G.loop()
    r = c.ref("random", c.strings[0])
    assert len(c.strings[0]) == G.LOOP_LEN and len(r.paths) == 1
    p = r.posterior
    assert p["counts"] == {c.model.pid[("H", "T", "H")]: 63.0, c.model.pid[("H", "T", G.END)]: 1.0}
    assert p["entropy"] == 0.0 and all(v == {c.model.sid["H"]: 1.0} for v in p["mass"]) and p["boundary"] == [1.0] * G.LOOP_LEN
    c, wn, s = G.ids65()
    counts = c.ref(wn, s).posterior["counts"]
    assert len(c.model.names) >= 66 and all(counts.get(j, 0.0) > 0.0 for j in (63, 64, 65))


# -- the id list names the path ----------------------------------------------------------------------

@pytest.mark.parametrize("name", list(G.CASES))
def test_paths_are_unique_by_id_list_and_orders_are_consistent(name):
    c = G.CASES[name]()
    for wn in c.weightings:
        for s in c.distinct:
            r = c.ref(wn, s)
            assert len({p.ids for p in r.paths}) == len(r.paths), (name, s)
            lw = [r.paths[l].lw for l in r.order]
            assert all(a >= b for a, b in zip(lw, lw[1:])) and sorted(r.order) == r.finite
            p = r.posterior
            if not r.finite:
                assert p["logq"] == -math.inf and r.mea([]) is None
                continue
            assert abs(p["logq"] - r.sample_logq) <= 1e-12 * max(1.0, abs(p["logq"]))
            assert all(abs(sum(row.values()) - 1.0) <= 1e-12 for row in p["mass"])
            assert r.L == 0 or abs(p["boundary"][-1] - 1.0) <= 1e-12
            l, score = r.mea(p["mass"])
            assert l in r.finite and abs(score - r.mea_score(l, p["mass"])) <= 1e-12 * max(1, r.L)
            assert all(score >= r.mea_score(k, p["mass"]) - 1e-12 * max(1, r.L) for k in r.finite[:200])


# -- the reference against the project's existing ones ---------------------------------------------------

@pytest.mark.parametrize("name", list(G.CASES))
def test_enumeration_is_the_enum_oracles(name):
    from oracle import ENUM, Oracle
    c = G.CASES[name]()
    wn = "random"
    strings = c.distinct
    mine = [c.ref(wn, s) for s in strings]

    def oracle(keep):
        sym = np.frombuffer(b"".join(keep), dtype=np.uint8).copy()
        off = np.concatenate([[0], np.cumsum([len(s) for s in keep])]).astype(np.int64)
        return Oracle.from_arrays(c.model.text, sym, off, np.ones(len(keep)), mode=ENUM, max_paths=10_000_000)
    assert [int(v) for v in oracle(strings).path_counts()] == [len(r.paths) for r in mine]
    o = oracle([r.s for r in mine if r.paths])
    names = o.param_names()
    col = {n: j for j, n in enumerate(names)}
    # the oracle trims a parameter no path uses and holds one fixed at 0 that is its state's only used one:
    # neither has a column, and the comparison runs at weights that are 0 there
    w = np.array([v if n in col else 0.0 for n, v in zip(c.model.names, c.weightings[wn])])
    rec = [G.Ref(c.model, r.s, w) for r in mine if r.paths]
    x = np.array([w[c.model.pid[n]] for n in names])
    prow, pcol, pdata, mrow = o.paths()
    for i, r in enumerate(rec):
        theirs = []
        for l in range(mrow[i], mrow[i + 1]):
            row = sorted((int(pcol[q]), int(pdata[q])) for q in range(prow[l], prow[l + 1]))
            with np.errstate(invalid="ignore"):
                theirs.append((row, float(sum(n * x[j] for j, n in row))))
        ours = [(sorted(collections.Counter(col[n] for n in _names(c.model, p.ids) if n in col).items()), p.lw) for p in r.paths]
        theirs.sort(key=lambda t: t[0])
        ours.sort(key=lambda t: t[0])
        assert [t[0] for t in theirs] == [t[0] for t in ours], (name, r.s)
        assert all(a[1] == b[1] or abs(a[1] - b[1]) <= _tol(b[1]) for a, b in zip(theirs, ours)), (name, r.s)


def test_posterior_is_the_marginal_references():
    c = G.composite()
    w = c.weightings["random"]
    en = MR.enumerate_corpus(c.model.fsa, c.sym, c.off)
    for s, entry in zip(c.strings, en["strings"]):
        r = c.ref("random", s)
        assert entry["n"] == len(r.paths)
        if not r.paths:
            continue
        d = MR.derive(entry, w, en["n_states"])
        p = r.posterior
        assert abs(d["logq"] - p["logq"]) <= 1e-12 * max(1.0, abs(p["logq"]))
        for i in range(r.L):
            got = np.zeros(en["n_states"])
            got[list(p["mass"][i])] = list(p["mass"][i].values())
            assert np.abs(got - d["mass"][i]).max() <= 1e-12 and abs(p["boundary"][i] - d["boundary"][i]) <= 1e-12
        counts = d["prob"] @ entry["C"][:, :len(w)].astype(np.float64)
        assert all(abs(counts[j] - p["counts"].get(j, 0.0)) <= 1e-12 * max(1.0, counts[j]) for j in range(len(w)))


def test_mea_is_not_viterbi_on_the_fixture():
    """test_gpu_byte_marginals' fixture (a): the most probable path is A's, the MEA decode B1 - C2 with score 0.95"""
    states = [(G.START, [""], ["A1", "B1"]), ("A1", ["x"], ["A2"]), ("A2", ["y"], [G.END]), ("B1", ["x"], ["C2", "D2"]),
              ("C2", ["y"], [G.END]), ("D2", ["y"], [G.END])]
    m = G.Model(states)
    r = G.Ref(m, b"xy", m.weights(FIXTURE_A_WEIGHTS))
    assert _names(m, r.paths[r.order[0]].ids) == [(G.START, "T", "A1")]
    l, score = r.mea(r.posterior["mass"])
    assert _names(m, r.paths[l].ids) == [(G.START, "T", "B1"), ("B1", "T", "C2")] and abs(score - 0.95) <= 1e-14


# -- the sampler's replay ------------------------------------------------------------------------------------

def test_replay_by_hand():
    """seam(65) at zero weights on xa: 65 equal end masses, so draw 0 takes the slot floor(65 u) and the
    one in-edge follows; the replayed paths are the reference's"""
    c = G.seam(65)
    r = c.ref("zero", b"xa")
    U = G.draws(G.SAMPLE_SEED, [0], 64, 2)
    which, ok = r.replay(U)
    assert ok.all()
    live = c.model.wide.slots[ord("a")]
    assert [r.paths[l].nodes[1] for l in which] == [live[int(math.floor(65 * u))] for u in U[:, 0]]
    assert len(set(which)) > 30


@pytest.mark.parametrize("name", list(G.CASES))
def test_no_sample_of_the_committed_seed_is_undecidable(name):
    c = G.CASES[name]()
    where = collections.defaultdict(list)
    for i, s in enumerate(c.strings):
        where[s].append(i)
    for wn in c.weightings:
        for s, idx in where.items():
            r = c.ref(wn, s)
            if not r.finite:
                continue
            which, ok = r.replay(G.draws(G.SAMPLE_SEED, idx, 64, r.L))
            assert ok.all(), (name, wn, s, int((~ok).sum()))
            assert set(which) <= set(r.finite)
