"""The numpy walker of wfsa_dev_generate's contract (generate_reference.py)
against the CPU oracle, without a GPU: every complete sample of the goldens and
of amb12 is a string the automaton recognizes, walked along one of the oracle's
enumerated paths of that string with that path's weight; on a tiny automaton
without a loop the walks' probabilities exp(logp) sum to 1 minus the dead mass;
and at group-normalised weights the reference's own samples pass the
distribution test test_gpu_generate.py puts to the device, for the seeds it
names and with no near-tie flag set -- which shows that the bound is fair."""
import os

import numpy as np
import pytest

import generate_reference as G
import sample_reference as R
from conftest import DATA
from decode_cases import _family, _tol

GOLDEN = ["test", "test5", "test.loop", "talk"]


def _text(name):
    if name in GOLDEN:
        return open(os.path.join(DATA, name + ".wfsa"), "rb").read().decode("latin-1")
    return _family(name)["text"]


def _oracle_paths(text, fsa, strings):
    """the oracle's enumerated paths of `strings` (distinct): P over its trimmed
    parameters, mrow, and the map from the Fsa's parameter ids to P's columns
    (-1: a parameter the oracle fixes, -2: one on no path)"""
    from oracle import Oracle
    from oracle.hessian import HessianOracle
    off = np.zeros(len(strings) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in strings], out=off[1:])
    sym = np.frombuffer(b"".join(strings), dtype=np.uint8)
    o = Oracle.from_arrays(text, sym, off, np.ones(len(strings)))
    assert (o.path_counts() > 0).all()   # every complete sample is recognized
    h = HessianOracle(o)
    names = {n: j for j, n in enumerate(o.full_param_names())}
    perm = np.array([names[n] for n in fsa.param_names()], dtype=np.int64)
    return h.P, np.asarray(h.mrow), o.trimmed_index()[perm]


@pytest.mark.parametrize("name", GOLDEN + ["amb12"])
def test_complete_samples_walk_oracle_paths(name):
    import wfsa_amd as W
    text = _text(name)
    fsa = W.Fsa.read_text(text)
    n_par = fsa.counts()["parameters"]
    for draw, w in enumerate([fsa.weights(), np.random.default_rng(7).normal(-1.0, 0.5, size=n_par)]):
        out = G.generate(fsa, w, 256, 8, seed=draw)
        done = np.flatnonzero(out["status"] == 0)
        assert len(done) > 0
        strs = G.strings(out)
        distinct = list(dict.fromkeys(strs[i] for i in done if len(strs[i]) > 0))
        if not distinct:
            continue
        P, mrow, col = _oracle_paths(text, fsa, distinct)
        x = np.zeros(P.shape[1])
        x[col[col >= 0]] = w[col >= 0]
        lw = R.path_weights(P, x)
        row_of = {s: r for r, s in enumerate(distinct)}
        for i in done:
            if not strs[i]:
                continue
            ids = out["pidx"][out["prow"][i]:out["prow"][i + 1]]
            c = col[ids]
            assert (c != -2).all()
            row = np.bincount(c[c >= 0], minlength=P.shape[1])
            r = row_of[strs[i]]
            hit = [l for l in range(mrow[r], mrow[r + 1]) if (P[l] == row).all()]
            assert hit, (name, i, strs[i], ids)
            # the oracle's weight of that path, plus the parameters it fixes and leaves out of P
            want = lw[hit[0]] + w[ids[c == -1]].sum()
            assert abs(want - out["logw"][i]) <= _tol(out["logw"][i]), (name, i, want, out["logw"][i])


def test_walk_probabilities_sum_to_one_minus_the_dead_mass():
    import wfsa_amd as W
    fsa = W.Fsa.read_text(G.TINY)
    w = G.normalised(fsa, fsa.weights())
    for dead in (False, True):
        ww = w.copy()
        lost = 0.0
        if dead:   # B's emissions at -inf: every walk that reaches B dies
            ww[G.params_of(fsa, "B", "E")] = -np.inf
            ta, tb, ab = (w[G.transition_param(fsa, u, v)] for u, v in (("^", "A"), ("^", "B"), ("A", "B")))
            lost = np.exp(tb) + np.exp(ta + ab)   # ^ -> B, and ^ -> A -> B whatever A emits
        out = G.generate(fsa, ww, 4096, 8, seed=5)
        assert not out["near"].any()
        assert (out["status"] != 1).all() and ((out["status"] == 2).any() == dead)
        walks = {}
        for i in np.flatnonzero(out["status"] == 0):
            walks[out["pidx"][out["prow"][i]:out["prow"][i + 1]].tobytes()] = out["logp"][i]
        total = np.exp(np.array(list(walks.values()))).sum()
        # 4,096 samples see every one of the at most 10 complete walks (the rarest has mass above 0.003)
        assert abs(total - (1.0 - lost)) <= 1e-12, (dead, total, lost)


@pytest.mark.parametrize("seed", G.DIST_SEEDS)
def test_reference_passes_the_distribution_test(seed):
    """the GPU test's statistic for the reference's own samples: log q_s of the
    distinct complete strings from the oracle's dense trellis at the same
    weights (the device test takes it from objective_grad)"""
    from oracle import Oracle, TRELLIS
    import wfsa_amd as W
    text, w = G.dist_model()
    fsa = W.Fsa.read_text(text)
    out = G.generate(fsa, w, G.DIST_N, G.DIST_MAX_LEN, seed)
    assert not out["near"].any()
    assert np.abs(out["logw"] - out["logp"]).max() <= 1e-12 * (out["steps"].max() + 1)
    strs = G.strings(out)
    counts = {}
    for i in np.flatnonzero(out["status"] == 0):
        counts[strs[i]] = counts.get(strs[i], 0) + 1
    distinct = list(counts)
    off = np.zeros(len(distinct) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in distinct], out=off[1:])
    o = Oracle.from_arrays(text, np.frombuffer(b"".join(distinct), dtype=np.uint8), off, np.ones(len(distinct)), mode=TRELLIS)
    names = {n: j for j, n in enumerate(fsa.param_names())}
    _, logq, _ = o.trellis_eval(w[[names[n] for n in o.full_param_names()]])
    assert np.isfinite(logq).all()   # no sample on a string of probability 0
    x2, dof = G.chi_square([counts[s] for s in distinct], G.DIST_N * np.exp(logq), int((out["status"] != 0).sum()), G.DIST_N)
    print("seed", seed, "X^2", x2, "dof", dof, "bound", R.bound(dof), "distinct", len(distinct))
    assert dof >= 100
    assert x2 <= R.bound(dof), (x2, dof)
