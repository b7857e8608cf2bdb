"""GPU tests of the second-order term H_f, entry by entry against the exact
covariance from enumerated paths in long double (tests/hf_reference.py):
hf_kernel (bubbles of compiled strings), hf_trav_kernel<R> (traversal
strings, every column tier vm = 64 R) and matrix-file mode's
mp_hf_slot_kernel + mp_hf_sum_kernel.  Every device value D[j,k] is held to

    |D - H| <= 1e-12 B,   D == 0 wherever B == 0

with B the same sum without its cancellation (hf_reference.py); the float64
restatement on the CPU stays within 1e-13 B (test_hf_reference.py).  Each
case prints its largest |D - H| / B.  Needs a gfx950 device."""
import numpy as np
import pytest

import hf_reference as R
from decode_cases import _device
from matrix_blocks_cases import _permute_rows

pytestmark = pytest.mark.gpu

TOL = R.TOL


def _report(impl, name, worst):
    print(f"hf_exact {impl} {name} max|D-H|/B {worst:.3e}")


def _vm(nv):
    vm = 64
    while vm < nv:
        vm *= 2
    return vm


def _automaton(name, monkeypatch):
    """the device over the case's whole corpus, its pattern mapped to the
    reference's trimmed parameters, and the column tier its traversal
    strings need"""
    ref = R.case(name)
    dev = _device(ref, monkeypatch)
    rec, pc, _ = dev.recognize()
    assert rec.all()
    np.testing.assert_array_equal(pc, np.diff(ref["mrow"]))
    tiers = dev.string_tiers()
    pairs = dev.hf_setup()
    t = ref["trim"][dev.perm]            # device parameter -> trimmed index
    tp = t[pairs]
    assert (tp >= 0).all()               # only parameters on paths take part
    nv = {s: len(eq) for s, eq in R.sets_of(name)}
    trav = [nv.get(s, 0) for s in np.flatnonzero(tiers >= 0)]
    return ref, dev, tiers, tp, (_vm(max(trav)) if trav else 0)


def _compare(impl, name, ref, evaluate, pairs, exact_pattern=False, label=None):
    """three weight draws of `evaluate(x) -> values` against the reference"""
    n = ref["o"].n
    worst, out = 0.0, []
    for x in R.draws(ref):
        H, B = R.hf_exact(ref["P"], ref["mrow"], ref["o"].p(), x, R.sets_of(name))
        D, seen = R.dense(n, pairs, evaluate(x))
        assert seen[B > 0].all(), "a pair of equivocal parameters is missing from the pattern"
        if exact_pattern:
            assert np.array_equal(seen, B > 0)
        worst = max(worst, R.worst_ratio(D, H, B))
        out.append((D, H, B))
    _report(impl, label or name, worst)
    assert worst <= TOL, worst
    return out


def _w(ref, dev, x):
    ref["o"].set_x(x)
    return ref["o"].w_full()[dev.perm]


@pytest.mark.parametrize("name,vm", [("amb12", 128), ("n16", 128)])
def test_random_families(name, vm, monkeypatch):
    """bubbles and traversal strings together; the largest V_s of a
    traversal string puts hf_trav_kernel on its vm = 128 tier"""
    ref, dev, tiers, tp, got_vm = _automaton(name, monkeypatch)
    assert (tiers == -1).any() and (tiers >= 0).any(), np.bincount(tiers + 1)
    assert got_vm == vm
    _compare(f"hf_kernel+hf_trav_kernel<{vm // 64}>", name, ref, lambda x: dev.hf_eval(_w(ref, dev, x)), tp)


@pytest.mark.parametrize("name,m_max,vm", [("ladder4x16", 16, 128), ("ladder4x17", 17, 256), ("ladder4x32", 32, 256),
                                           ("ladder4x64", 64, 512)])
def test_ladder_tier_boundaries(name, m_max, vm, monkeypatch):
    """K = 4 chains: max |V_s| = 8 m_max sits exactly at a column tier's
    limit (128, 256, 512 = kHfTravMaxV) or just over one (136).  Strings up
    to length 7 (4 m + 2 = 30 nodes) compile into bubbles, longer ones run
    on the traversal tiers"""
    ref, dev, tiers, tp, got_vm = _automaton(name, monkeypatch)
    lens = np.diff(ref["off"])
    assert (tiers[lens <= 7] == -1).all() and (tiers[lens >= 8] >= 0).all(), (tiers, lens)
    assert got_vm == vm
    _compare(f"hf_kernel+hf_trav_kernel<{vm // 64}>", name, ref, lambda x: dev.hf_eval(_w(ref, dev, x)), tp)


def test_ladder_at_the_bubble_node_limit(monkeypatch):
    """K = 3, m_max = 10: the longest strings' region has 3 * 10 + 2 = 32
    nodes, kMaxBubbleNodes: it still compiles, nothing is left to the
    traversal tiers"""
    ref, dev, tiers, tp, got_vm = _automaton("ladder3x10", monkeypatch)
    assert (tiers == -1).all(), tiers
    _compare("hf_kernel", "ladder3x10", ref, lambda x: dev.hf_eval(_w(ref, dev, x)), tp)


def test_scratch_reuse(monkeypatch):
    """816 traversal strings at vm = 512 over 258 nodes: a wave's scratch is
    806,875 doubles, the 2 GiB budget holds 332 of them, so every wave
    carries two or three strings through the same scratch (hf_trav_kernel's
    `li += nwv` loop); and the evaluation repeats bit for bit"""
    name = "ladder4x64_700"
    ref, dev, tiers, tp, got_vm = _automaton(name, monkeypatch)
    assert got_vm == 512 and (tiers >= 0).sum() == 816
    # hf_setup's wave count is min(strings, 8 per CU, 2 GiB / hf_trav_stride doubles): fewer than half the strings
    st = dev.stats()
    N, L, vm = st["n_nodes"], st["max_len"], 512
    assert (N, L) == (258, 64)
    stride = (L + 1) * (N + 1) + 4 * N + 2 * N * vm + 2 * vm * vm + vm + 16     # fb_kernels.hpp hf_trav_stride
    assert stride == 806875 and ((2 << 30) // 8) // stride == 332 < 816 // 2
    _compare("hf_kernel+hf_trav_kernel<8>", name, ref, lambda x: dev.hf_eval(_w(ref, dev, x)), tp)
    w = _w(ref, dev, R.draws(ref)[0])
    assert dev.hf_eval(w).tobytes() == dev.hf_eval(w).tobytes()


def _matrix_device(ref, permuted):
    """the case's path matrices on the device; permuted: the paths stored in
    a random order (P's rows permuted), M's columns naming them"""
    import wfsa_amd as W
    o = ref["o"]
    prow, pcol, pdata, mrow = o.paths()
    n_paths = len(prow) - 1
    mcol = np.arange(n_paths)
    if permuted:
        mcol = np.random.default_rng(17).permutation(n_paths)     # path k of M order is P row mcol[k]
        prow, pcol, pdata = _permute_rows(prow, pcol, pdata, mcol)
    dev = W.Device(0)
    dev.load_paths(o.n, prow, pcol, pdata, mrow, mcol, o.p())
    return dev


@pytest.mark.parametrize("permuted", [False, True], ids=["identity", "permuted"])
@pytest.mark.parametrize("name", ["amb12", "ladder4x32"])
def test_matrix_mode(name, permuted):
    """mp_hf_slot_kernel + mp_hf_sum_kernel over more than 256 slots and
    more than 256 pairs (several blocks of both): the pattern is exactly
    {B > 0, j <= k}, the values pass the rule"""
    ref = R.case(name)
    dev = _matrix_device(ref, permuted)
    pairs = dev.hf_setup()
    assert len(pairs) > 256 and (pairs[:, 0] <= pairs[:, 1]).all()
    _compare("mp_hf", name, ref, dev.hf_eval, pairs, exact_pattern=True, label=name + ("+permuted" if permuted else ""))


def test_three_implementations_agree(monkeypatch):
    """amb12: the automaton's bubbles + traversal strings and matrix-file
    mode (both path orders) within 2e-12 B of each other"""
    name = "amb12"
    ref, dev, tiers, tp, _ = _automaton(name, monkeypatch)
    n = ref["o"].n
    m0, m1 = _matrix_device(ref, False), _matrix_device(ref, True)
    p0, p1 = m0.hf_setup(), m1.hf_setup()
    for x in R.draws(ref):
        _, B = R.hf_exact(ref["P"], ref["mrow"], ref["o"].p(), x, R.sets_of(name))
        Da, _ = R.dense(n, tp, dev.hf_eval(_w(ref, dev, x)))
        D0, _ = R.dense(n, p0, m0.hf_eval(x))
        D1, _ = R.dense(n, p1, m1.hf_eval(x))
        for U, V in ((Da, D0), (Da, D1), (D0, D1)):
            assert (np.abs(U - V) <= 2e-12 * B).all()


def _eps_ladder(n_eps):
    """the K = 4, m_max = 9 ladder with n_eps epsilon states (each with a way
    on and a way to `$`, so each transition is a parameter) between c0_3 and
    c0_4: one combined edge of chain 0 carries n_eps + 2 parameters"""
    lines = R.ladder_text(4, 9).split("\n")
    i = lines.index("c0_3 c0_4 0 $ 0")
    chain = [f"e{q}" for q in range(n_eps)]
    lines[i] = f"c0_3 {chain[0]} 0 $ 0"
    extra = []
    for q, e in enumerate(chain):
        extra += [f"{e}  0", f"{e} {chain[q + 1] if q + 1 < n_eps else 'c0_4'} 0 $ 0"]
    return "\n".join(lines[:i + 1] + extra + lines[i + 1:])


def test_traversal_edge_with_more_than_8_parameters():
    """an epsilon chain folds into its combined edge; hf_trav_kernel collects
    at most 8 equivocal parameters of one edge, so hf_setup refuses a
    traversal string that has more on one (as it does for bubble edges).
    Only strings of 8 and 9 bytes (34 and 38 nodes: no bubble holds them),
    so the refusal is the traversal strings' own"""
    import wfsa_amd as W
    sym, off, wt = R._pack([b"abababab", b"babababab", b"aaaaaaaaa", b"bbbbbbbbb"])
    dev = W.Device(0)
    dev.load_model(W.Fsa.read_text(_eps_ladder(9)))
    dev.load_corpus(sym, off, wt / wt.sum())
    rec, _, _ = dev.recognize()
    assert rec.all() and (dev.string_tiers() >= 0).all()
    with pytest.raises(W.WfsaError, match="more than 8 of them equivocal") as e:
        dev.hf_setup()
    assert e.value.code == W._lib.WFSA_ERR_CAPACITY


def test_traversal_edge_with_8_parameters(monkeypatch):
    """the same ladder with an edge of exactly 8 parameters, over the whole
    ladder corpus (nothing on a path trimmed): accepted, and exact"""
    from decode_cases import _reference
    ref = _reference(_eps_ladder(6), *R._pack(R.ladder_corpus(9)))
    assert not (ref["trim"] == -1).any() and len(ref["rec"]) == len(ref["off"]) - 1
    dev = _device(ref, monkeypatch)
    rec, _, _ = dev.recognize()
    assert rec.all() and (dev.string_tiers() >= 0).sum() >= 4
    tp = ref["trim"][dev.perm][dev.hf_setup()]
    assert (tp >= 0).all()
    sets = R.equivocal_sets(ref["P"], ref["mrow"])
    worst = 0.0
    for x in R.draws(ref):
        H, B = R.hf_exact(ref["P"], ref["mrow"], ref["o"].p(), x, sets)
        D, seen = R.dense(ref["o"].n, tp, dev.hf_eval(_w(ref, dev, x)))
        assert seen[B > 0].all()
        worst = max(worst, R.worst_ratio(D, H, B))
    _report("hf_kernel+hf_trav_kernel<2>", "ladder4x9+eps6", worst)
    assert worst <= TOL, worst
