"""CPU checks of the long-double H_f reference (tests/hf_reference.py) and of
the shapes the GPU tests rely on: the float64 restatement
(oracle/hessian.py HessianOracle.hf) stays within 1e-13 B of it -- ten times
inside the 1e-12 B the device is held to --, every case shows the largest
|V_s| its column tier needs, every string is recognized, and no parameter on
a path is trimmed away (so no device pair is left out of a comparison)."""
import copy

import numpy as np
import pytest

import hf_reference as R


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_shape(name):
    ref = R.case(name)
    o, P, mrow, trim = ref["o"], ref["P"], ref["mrow"], ref["trim"]
    n_corpus = len(ref["off"]) - 1
    # every string recognized: the device's p (weights / their sum) is the oracle's
    assert len(ref["rec"]) == n_corpus == len(mrow) - 1
    np.testing.assert_allclose(o.p(), ref["wt"] / ref["wt"].sum(), rtol=1e-15)
    # nothing on a path is trimmed: every Fsa parameter is unused (-2) or kept
    assert not (trim == -1).any()
    assert (P.sum(axis=0) > 0).all() and (trim >= 0).sum() == P.shape[1]
    sets = R.sets_of(name)
    assert max(len(eq) for _, eq in sets) == R.CASES[name][1]
    h = ref["h"]
    assert len(sets) == len(h.equivocal)
    for (s, eq), (s2, eq2) in zip(sets, h.equivocal):
        assert s == s2 and np.array_equal(eq, eq2)


@pytest.mark.parametrize("name,K,m_max", [("ladder4x16", 4, 16), ("ladder4x17", 4, 17), ("ladder4x32", 4, 32),
                                          ("ladder4x64", 4, 64), ("ladder3x10", 3, 10), ("ladder4x64_700", 4, 64)])
def test_ladder_facts(name, K, m_max):
    """a string of length m has exactly K paths with pairwise distinct
    parameters, all equivocal: the branch out of `^`, m emissions and m
    transitions on each, |V_s| = K (2 m + 1) -- but a chain's last state has
    `$` as its only transition, which is no parameter, so |V_s| = 2 K m_max
    at m = m_max, the largest of the case"""
    ref = R.case(name)
    P, mrow, off = ref["P"], ref["mrow"], ref["off"]
    lens = np.diff(off)[ref["rec"]]
    assert (np.diff(mrow) == K).all()
    assert lens.min() >= 1 and lens.max() == m_max
    sets = R.sets_of(name)
    assert len(sets) == len(lens)
    for s, eq in sets:
        rows = P[mrow[s]:mrow[s + 1]]
        m = lens[s]
        assert len(eq) == (2 * K * m if m == m_max else K * (2 * m + 1))
        assert ((rows > 0).sum(axis=0) <= 1).all() and rows.max() == 1
    if name == "ladder4x64_700":
        assert len(lens) >= 700 and lens[:700].min() == 8


@pytest.mark.parametrize("name", list(R.CASES))
def test_float64_restatement_within_1e13(name):
    ref = R.case(name)
    h = copy.copy(ref["h"])
    worst = 0.0
    # the 700-string ladder is the slow one (830 dense 512 x 512 blocks a draw): one draw here
    for x in R.draws(ref)[:1 if name == "ladder4x64_700" else 3]:
        H, B = R.hf_exact(ref["P"], ref["mrow"], ref["o"].p(), x, R.sets_of(name))
        assert np.array_equal(B > 0, B.T > 0)
        pat = np.zeros(B.shape, dtype=bool)
        for _, eq in R.sets_of(name):
            pat[np.ix_(eq, eq)] = True
        assert np.array_equal(B > 0, pat)     # B > 0 exactly on the union of V_s x V_s
        h.x = x
        _, rpp = h.modeled()
        worst = max(worst, R.worst_ratio(-h.hf(rpp), H, B))
    print(f"{name}: float64 restatement within {worst:.2e} B of the long-double reference")
    assert worst <= 1e-13
