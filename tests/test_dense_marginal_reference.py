"""CPU checks of the numpy restatement of the dense path's byte marginals and
MEA decode (dense_marginal_reference.py), which the GPU tests compare the
device against: its masses and log q against a plain enumeration of the
accepting paths (marginal_reference.py) on the 5-state forced-dense case, its
decode against the enumerated paths' scores, and that the decode matters on the
project's dense cases (the MEA path is not the Viterbi path)."""
import numpy as np
import pytest

import dense_decode_reference as R
import dense_marginal_reference as M
import dense_sample_reference as D
import marginal_reference as MR


@pytest.fixture(scope="module", autouse=True)
def _drop():
    yield
    M.clear_caches()


def _five_states():
    import wfsa_amd as W
    syn = W.Synthetic(n_states=5, degree=1, vocab=3, emissions=2, dense=True, n_strings=60, max_len=5, seed=9)
    sym, off, wt = syn.corpus()
    fsa = W.Fsa.read_text(syn.wfsa_text)
    w = np.random.default_rng(5).normal(-1.0, 0.7, size=len(fsa.param_names()))
    return fsa, w, sym, off


def test_masses_and_logq_against_the_enumerated_paths():
    """masses and log q to 1e-12; every byte's masses sum to 1; the replay's
    score is the greatest enumerated score to 1e-12 and its path an enumerated
    path carrying that score"""
    fsa, w, sym, off = _five_states()
    enum = MR.enumerate_corpus(fsa, sym, off)
    ids = M.state_ids(fsa)
    tab = R.Tables(fsa, w)
    logq, masses = M.corpus(fsa, w, sym, off)
    seen = 0
    for s, entry in enumerate(enum["strings"]):
        d = MR.derive(entry, w, enum["n_states"])
        assert np.isfinite(d["logq"]) and entry["n"] > 0
        assert abs(logq[s] - d["logq"]) <= 1e-12 * max(1.0, abs(d["logq"]))
        L = entry["L"]
        full = np.zeros((L, enum["n_states"]))
        full[:, ids] = masses[s]
        assert np.abs(full - d["mass"]).max(initial=0.0) <= 1e-12
        assert np.abs(masses[s].sum(axis=1) - 1.0).max(initial=0.0) <= 1e-12
        bytes_ = sym[off[s]:off[s + 1]]
        states, pids, score, plw = M.mea_replay(tab, bytes_, masses[s])
        assert abs(score - d["best"]) <= 1e-12
        match = [l for l in range(entry["n"]) if list(entry["params"][l]) == list(pids)]
        assert match, (s, pids)
        assert any(abs(d["score"][l] - d["best"]) <= 1e-12 and np.array_equal(ids[states], entry["states"][l]) for l in match)
        assert abs(plw - d["lw"][match[0]]) <= 1e-12 * max(1.0, abs(plw))
        assert np.array_equal(M.path_states(tab, bytes_, pids), states) or len(match) > 1
        seen += entry["n"] > 1
    assert seen >= 20   # (ambiguous strings)


def test_the_mea_path_is_not_the_viterbi_path_on_dense16():
    """for at least one string the replayed MEA path differs from decode()'s
    and scores higher there; it never scores lower"""
    fsa, w, sym, off, p, tab, logq, masses = M.expected("dense16")
    differ, gain = 0, 0.0
    for s in range(len(off) - 1):
        bytes_ = sym[off[s]:off[s + 1]]
        states, pids, score, plw = M.mea_replay(tab, bytes_, masses[s])
        vlw, vids, _, _ = R.decode(tab, bytes_)
        vscore = M.path_score(masses[s], M.path_states(tab, bytes_, vids))
        assert score >= vscore - 1e-12 and plw <= vlw + 1e-12
        if not np.array_equal(pids, vids):
            differ += 1
            gain = max(gain, score - vscore)
    print("dense16: MEA path differs from the Viterbi path on", differ, "of", len(off) - 1, "strings; largest gain", gain)
    assert differ >= 1 and gain > 1e-6


def test_without_a_path_case_has_both_kinds():
    fsa, w, sym, off, p, tab, logq, masses = M.expected("without_a_path")
    none = np.isneginf(logq)
    assert none[-1] and none.any() and (~none).any()
    assert np.array_equal(none, np.isneginf(D.sample_corpus(fsa, w, sym, off, 1, 1)[4]))
    for s in np.flatnonzero(none):
        assert masses[s] is None or masses[s].shape[0] == 0
        assert np.isnan(M.mea_replay(tab, sym[off[s]:off[s + 1]], None)[2])
    for s in np.flatnonzero(~none):
        if off[s + 1] > off[s]:
            assert np.abs(masses[s].sum(axis=1) - 1.0).max() <= 1e-12
            states, pids, score, plw = M.mea_replay(tab, sym[off[s]:off[s + 1]], masses[s])
            assert np.isfinite(w[pids]).all() and 0.0 < score <= len(states) * (1.0 + 1e-12)


def test_the_clamp_and_the_listing_rule():
    """min(gamma, 1.0), listed when > 0: a denormal is listed, 0.0 and -0.0
    are not, a value above 1 is stored as 1.0"""
    idx, val = M.stored_row([0.0, 5e-324, 0.5, 1.0 + 2.0 ** -40, -0.0, 1.0])
    assert list(idx) == [1, 2, 3, 5]
    assert val.tobytes() == np.array([5e-324, 0.5, 1.0, 1.0]).tobytes()
    # the replay reads an unlisted state as 0.0 and never takes an ineligible one
    fsa, w, sym, off, p, tab, logq, masses = M.expected("dense16")
    s = int(np.argmax(np.diff(off)))
    bytes_ = sym[off[s]:off[s + 1]]
    stored = np.zeros_like(masses[s])
    for j in range(len(bytes_)):
        i, v = M.stored_row(masses[s][j])
        stored[j, i] = v
    states, pids, score, plw = M.mea_replay(tab, bytes_, stored)
    assert score == M.path_score(stored, states)
    assert all(tab.pE[T, b] != -2 for T, b in zip(states, bytes_))
