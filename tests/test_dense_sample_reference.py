"""CPU checks of the numpy restatement of the dense path's posterior sampler
(dense_sample_reference.py), which the GPU tests compare the device against:
its paths and their distribution against the oracle's enumerated paths on the
5-state forced-dense case, and the condition that makes the GPU tests'
path-for-path comparison a fair demand -- for every (case, n) they compare,
under 1% of the samples have a choice closer than 1e-9 (relative to the total)
to a running-sum boundary, where the device's grouped sums and the plain ones
differ by about L np eps ~ 1e-12 (np <= 256, L <= 40; long300: np = 128)."""
import numpy as np
import pytest

import dense_sample_reference as D
import sample_reference as SR


def test_restatement_against_the_oracles_enumerated_paths():
    """every sampled path is an enumerated path of its string with the
    oracle's weight, exp(logw - logq) is its posterior mass, and 64 samples x
    16 seeds per string pass sample_reference's goodness-of-fit test"""
    import wfsa_amd as W
    from decode_cases import _reference, _tol
    syn = W.Synthetic(n_states=5, degree=1, vocab=3, emissions=2, dense=True, n_strings=60, max_len=5, seed=9)
    sym, off, wt = syn.corpus()
    ref = _reference(syn.wfsa_text, sym, off, wt)
    fsa = W.Fsa.read_text(syn.wfsa_text)
    o = ref["o"]
    names = {n: j for j, n in enumerate(o.full_param_names())}
    perm = np.array([names[n] for n in fsa.param_names()], dtype=np.int64)
    S = len(off) - 1
    assert len(ref["rec"]) == S
    x = SR.dist_weights(ref)
    o.set_x(x)
    w = o.w_full()[perm]
    P, mrow, trim = ref["P"], ref["mrow"], ref["trim"]
    lw = SR.path_weights(P, x)
    cells = SR.posterior_cells(ref, x)
    counts = [np.zeros(len(prob)) for _, prob, _ in cells]
    weights_of = []   # per string: count row -> the oracle weights of the paths with that row
    for r in range(len(mrow) - 1):
        by_row = {}
        for l in range(mrow[r], mrow[r + 1]):
            by_row.setdefault(P[l].astype(np.int64).tobytes(), []).append(lw[l])
        weights_of.append(by_row)
    for seed in SR.DIST_SEEDS:
        srow, logw, prow, pidx, logq, margin = D.sample_corpus(fsa, w, sym, off, SR.DIST_N, seed)
        assert (np.diff(srow) == SR.DIST_N).all() and np.isfinite(logq).all()
        for r, s in enumerate(ref["rec"]):
            a, b = mrow[r], mrow[r + 1]
            assert abs(logq[s] - SR.logsumexp(lw[a:b])) <= _tol(logq[s])
            keys = cells[r][0]
            for t in range(srow[s], srow[s + 1]):
                ids = pidx[prow[t]:prow[t + 1]]
                tr = trim[perm[ids]]
                assert (tr != -2).all()
                row = np.bincount(tr[tr >= 0], minlength=P.shape[1]).astype(np.int64)
                key = row.tobytes()
                assert key in keys, (s, t, ids)   # an enumerated path of this string
                assert any(abs(v - logw[t]) <= _tol(logw[t]) for v in weights_of[r][key]), (s, t)
                assert logw[t] - logq[s] <= _tol(logq[s])
                counts[r][keys[key]] += 1
    n = SR.DIST_N * len(SR.DIST_SEEDS)
    x2, dof, impossible = SR.chi_square(cells, counts, n)
    print("dense sample restatement: X^2", x2, "dof", dof, "bound", SR.bound(dof))
    assert dof >= 50
    assert impossible == 0 and x2 <= SR.bound(dof)


def test_first_samples_do_not_depend_on_n():
    fsa, w, sym, off, p = D.case("dense16")
    sub_off = off[:41]   # the first 40 strings
    a = D.sample_corpus(fsa, w, sym, sub_off, 2, 5)
    b = D.sample_corpus(fsa, w, sym, sub_off, 6, 5)
    for s in range(40):
        for t in range(2):
            i, j = a[0][s] + t, b[0][s] + t
            assert a[1][i] == b[1][j]
            assert np.array_equal(a[3][a[2][i]:a[2][i + 1]], b[3][b[2][j]:b[2][j + 1]])


@pytest.mark.parametrize("name,n", D.PATH_CASES, ids=lambda v: str(v))
def test_path_comparison_cases_have_wide_choices(name, n):
    """the GPU tests demand the restatement's paths (and the trellis sampler's)
    of every sample whose margin is at least 1e-9: fewer than 1% may fall below"""
    srow, logw, prow, pidx, logq, margin = D.expected(name, n)
    assert len(margin) > 0
    share = float((margin < D.MARGIN).mean())
    print(name, n, "samples", len(margin), "exempt share", share, "smallest margin", margin.min())
    assert share < D.EXEMPT


def test_without_a_path_case_has_both_kinds():
    fsa, w, sym, off, p = D.without_a_path_case()
    srow, logw, prow, pidx, logq, margin = D.sample_corpus(fsa, w, sym, off, 3, 1)
    none = np.isneginf(logq)
    assert none[-1] and none.any() and (~none).any()
    assert (np.diff(srow)[none] == 0).all() and (np.diff(srow)[~none] == 3).all()
    assert np.isfinite(w[pidx]).all()
