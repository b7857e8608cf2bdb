"""CPU tests of the reference the byte-marginal tests rest on
(marginal_reference.py), on the golden models and amb12, compiled64, long64:
the plain enumeration finds as many accepting paths per string as the oracle
counts, its log q and expected parameter counts are the oracle-based E-step's
(posterior_reference.posterior) to 1e-12, every byte's masses sum to 1 and the
last byte is a boundary; and on the hand-made fixture the most probable path is
not the analysis with the most bytes right in expectation."""
import functools

import numpy as np
import pytest

import marginal_reference as MR
import posterior_reference as PR
from decode_cases import GOLDEN, _source
from test_gpu_byte_marginals import FIXTURE_A, FIXTURE_A_WEIGHTS, fixture_weights

CASES = [c[0] for c in GOLDEN] + ["amb12", "compiled64", "long64"]


@functools.lru_cache(maxsize=None)
def _case(name):
    """the enumeration in the library's numbering, the map from its parameter
    ids to the oracle's columns, one weight draw and the oracle-based E-step there"""
    import wfsa_amd as W
    ref = _source(name)
    fsa = W.Fsa.read_text(ref["text"])
    en = MR.enumerate_corpus(fsa, ref["sym"], ref["off"])
    o = ref["o"]
    names = {n: j for j, n in enumerate(o.full_param_names())}
    perm = np.array([names[n] for n in fsa.param_names()], dtype=np.int64)
    x = np.random.default_rng(5).normal(-1.0, 0.5, size=o.n)
    o.set_x(x)
    return ref, en, perm, o.w_full()[perm], PR.posterior(ref, x)


@pytest.mark.parametrize("name", CASES)
def test_path_counts_are_the_oracles(name):
    ref, en, _, _, _ = _case(name)
    assert [e["n"] for e in en["strings"]] == [int(v) for v in ref["o"].path_counts()]
    assert sum(e["n"] for e in en["strings"]) == ref["P"].shape[0]


@pytest.mark.parametrize("name", CASES)
def test_logq_and_expected_counts_are_the_e_steps(name):
    ref, en, perm, w, (want_lq, want_c, _) = _case(name)
    col = ref["trim"][perm]   # the library's parameter id -> the oracle's column (< 0: none)
    worst = [0.0, 0.0]
    for r, s in enumerate(ref["rec"]):
        entry = en["strings"][s]
        d = MR.derive(entry, w, en["n_states"])
        counts = d["prob"] @ entry["C"][:, :len(col)].astype(np.float64)
        assert (col[counts > 0] != -2).all()   # no unused parameter on a path
        got = np.zeros(want_c.shape[1])
        np.add.at(got, col[col >= 0], counts[col >= 0])
        worst[0] = max(worst[0], abs(d["logq"] - want_lq[r]) / max(1.0, abs(want_lq[r])))
        worst[1] = max(worst[1], (np.abs(got - want_c[r]) / np.maximum(1.0, want_c[r])).max())
    print(name, "worst log q and count differences:", worst)
    assert worst[0] <= 1e-12 and worst[1] <= 1e-12


@pytest.mark.parametrize("name", CASES)
def test_masses_sum_to_one_and_the_last_byte_is_a_boundary(name):
    ref, en, _, w, _ = _case(name)
    for s in ref["rec"]:
        entry = en["strings"][s]
        d = MR.derive(entry, w, en["n_states"])
        if entry["L"] == 0:
            continue
        assert np.abs(d["mass"].sum(axis=1) - 1.0).max() <= 1e-12, s
        assert abs(d["boundary"][-1] - 1.0) <= 1e-12 and (d["boundary"] <= 1.0 + 1e-12).all(), s
        assert 0.0 < d["best"] <= entry["L"] + 1e-12, s


def test_the_fixtures_mea_path_is_not_its_viterbi_path():
    import wfsa_amd as W
    fsa = W.Fsa.read_text(FIXTURE_A)
    w = fixture_weights(fsa, FIXTURE_A_WEIGHTS)
    en = MR.enumerate_corpus(fsa, np.frombuffer(b"xy", dtype=np.uint8), np.array([0, 2]))
    entry = en["strings"][0]
    d = MR.derive(entry, w, en["n_states"])
    names = fsa.state_names()
    by_states = {tuple(names[u] for u in entry["states"][l]): l for l in range(entry["n"])}
    assert set(by_states) == {("A1", "A2"), ("B1", "C2"), ("B1", "D2")}
    a, c, dd = by_states[("A1", "A2")], by_states[("B1", "C2")], by_states[("B1", "D2")]
    assert np.allclose(d["prob"][[a, c, dd]], [0.40, 0.35, 0.25], rtol=0, atol=1e-15)
    assert np.allclose(d["score"][[a, c, dd]], [0.80, 0.95, 0.85], rtol=0, atol=1e-15)
    assert int(np.argmax(d["lw"])) == a and int(np.nanargmax(d["score"])) == c
    assert abs(d["logq"]) <= 1e-15 and np.abs(d["boundary"] - 1.0).max() <= 1e-15
