"""CPU checks of the numpy restatement of the dense path's Viterbi decode
(dense_decode_reference.py), which the GPU tests compare the device against:
brute-force path enumeration on a 4-state dense model, and the condition that
makes the GPU tests' byte-for-byte comparison with the trellis decode a fair
demand -- for each of those (model, weight draw) cases every decision on every
returned path is wider than 1e-9 and none is an exact tie, where the two decoders' roundings differ by
~1e-15 (they round (D + lA) + lE and D + (lA + lE))."""
import itertools

import numpy as np

import dense_decode_reference as R


def _brute(tab, s):
    """(best weight, the set of maximising state sequences' id tuples) by enumeration"""
    if len(s) == 0:
        return (tab.lse, {tuple([tab.pse] if tab.pse >= 0 else [])}) if tab.lse > -np.inf else (-np.inf, set())
    best, arg = -np.inf, []
    for st in itertools.product(range(tab.n), repeat=len(s)):
        v = tab.l0[st[0]] + tab.lE[st[0], s[0]]
        for j in range(1, len(s)):
            v += tab.lA[st[j - 1], st[j]] + tab.lE[st[j], s[j]]
        v += tab.lend[st[-1]]
        if v > -np.inf:
            arg.append((v, st))
            best = max(best, v)
    tol = 1e-12 * max(1.0, abs(best)) if best > -np.inf else 0.0
    paths = set()
    for v, st in arg:
        if best - v <= tol:
            ids = []
            for j, T in enumerate(st):
                ids += [tab.p0[T] if j == 0 else tab.pA[st[j - 1], T], tab.pE[T, s[j]]]
            ids.append(tab.pend[st[-1]])
            paths.add(tuple(int(p) for p in ids if p >= 0))
    return best, paths


def test_reference_against_path_enumeration():
    """a 4-state dense model, every string of length <= 4 over its bytes (and
    one byte nobody emits), three weight draws, one with -inf parameters:
    best weight within 1e-12 max(1, |v|), the path among the maximisers"""
    import wfsa_amd as W
    syn = W.Synthetic(n_states=4, degree=1, vocab=3, emissions=2, dense=True, n_strings=10, max_len=4, seed=7)
    fsa = W.Fsa.read_text(syn.wfsa_text)
    n_par = len(fsa.param_names())
    rng = np.random.default_rng(1)
    probe = R.Tables(fsa, np.zeros(n_par))
    assert probe.n == 4
    alphabet = [int(b) for b in np.flatnonzero((probe.pE != -2).any(axis=0))] + [255]
    strings = [s for L in range(5) for s in itertools.product(alphabet, repeat=L)]
    seen_none = seen_path = 0
    for draw in range(3):
        w = rng.normal(-1.0, 0.5, size=n_par)
        if draw == 2:
            w[rng.choice(n_par, size=n_par // 4, replace=False)] = -np.inf
        tab = R.Tables(fsa, w)
        for s in strings:
            want, paths = _brute(tab, s)
            got, ids, gap, _ = R.decode(tab, np.array(s, dtype=np.int64))
            if want == -np.inf:
                assert got == -np.inf and len(ids) == 0
                seen_none += 1
                continue
            assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (s, got, want)
            assert tuple(int(p) for p in ids) in paths, (s, ids)
            assert np.isfinite(w[ids]).all() and gap >= 0.0
            seen_path += 1
    assert seen_none > 100 and seen_path > 100


def test_byte_comparison_cases_have_wide_decisions():
    """the GPU tests demand byte equality with the trellis decode for these
    cases: no decision on a returned path may be closer than 1e-9 or tied"""
    import wfsa_amd as W
    for name in R.BYTE_CASES:
        text, sym, off, wt = R.synthetic(name)
        fsa = W.Fsa.read_text(text)
        w = R.case_weights(name, len(fsa.param_names()))
        logw, prow, pidx, gaps, ties = R.decode_corpus(fsa, w, sym, off)
        assert np.isfinite(logw).all()
        print(name, "smallest on-path gap", gaps.min(), "exact ties on a path", ties.sum())
        assert gaps.min() > 1e-9, (name, gaps.min(), int(np.argmin(gaps)))
        # the gap is between DISTINCT values: a candidate equal to the best to the bit (another order of the same
        # edges) is a decision of width 0 that the trellis decode's rounding may take the other way
        assert ties.sum() == 0, (name, np.flatnonzero(ties))
