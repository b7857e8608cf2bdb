"""The five wave-per-string trellis walkers -- best_path_kernel,
kbest_kernel<KC>, sample_path_kernel, posterior_counts_kernel and
marginal_rows_kernel / marginal_decode_kernel -- on automata built by hand
(trellis_gadgets.py), against a reference that knows paths as edge sequences.

The walkers' other tests accept a returned path when SOME oracle path has its
parameter count row; here every case names each path by its id list in path
order, so the documented total orders (decode.hpp, marginals.hpp) are held
path for path: live sets of exactly 63, 64, 65, 128 and 129 slots at the last
position and in the middle, ragged in-edge and end-edge counts across the lanes
of one round, counts on the parameter ids 63, 64 and 65, a corpus in which a
score, a gamma or a count left behind by one string would change the next
one's answer by 40, strings that die at every stage, and the empty string.

Per case ONE device runs all five walkers at every weighting (WFSA_DENSE=0);
the test functions read that one set of results.
  best_paths      the reference's first path, exactly; weight within _tol
  kbest_paths     k in 1, 2, 3, 4, 5, 8, 16: the first min(k, m) paths of the
                  total order, in order; k = j is the byte prefix of k = 16;
                  k = 1 carries best_paths' bytes
  sample_paths    n in 1, 64: EVERY sample is the replayed walk of its uniforms
                  (test_trellis_gadgets_reference.py shows none is undecidable);
                  weights carry kbest_paths' bytes; log q within
                  1e-11 max(1, |log q|)
  posterior_counts  exactly the parameters of positive count; counts and
                  entropy within posterior_reference.cap; sample_paths' log q
                  bytes; single-path strings exact; the same bytes again
  byte_marginals  masses and boundaries within cap, exactly the states of
                  positive mass, sums within cap of 1; the MEA path is the
                  reference's first in marginals.hpp's order under the masses
                  the device stored; its weight carries kbest_paths' bytes; its
                  score within L cap of the path's exact score
Equal strings give equal bytes and a second call gives the same bytes, on every
walker.  No tolerance here is new.  The worst errors per walker are printed as
one JSON line when the module ends (profiles/trellis_gadgets/errors.json).
Needs a gfx950 device."""
import collections
import json
import math
import os

import numpy as np
import pytest

import posterior_reference as PR
import trellis_gadgets as G
from decode_cases import _tol

pytestmark = pytest.mark.gpu

NS = (1, 64)
EXACT = ("few1", "loop")   # one path: counts, entropy and masses come out exact
ERRORS = collections.defaultdict(dict)
_RUNS = {}


@pytest.fixture(scope="module", autouse=True)
def _report_and_drop():
    yield
    print("trellis_gadgets errors " + json.dumps({k: ERRORS[k] for k in sorted(ERRORS)}, sort_keys=True))
    _RUNS.clear()
    G.clear_caches()


def _note(walker, **errs):
    for k, v in errs.items():
        ERRORS[walker][k] = max(ERRORS[walker].get(k, 0.0), float(v))


def _run(name):
    """the case on one device: every walker at every weighting, twice where the
    second call's bytes are compared -- computed once and left unchanged"""
    if name in _RUNS:
        return _RUNS[name]
    import wfsa_amd as W
    c = G.CASES[name]()
    saved = {k: os.environ.get(k) for k in ("WFSA_DENSE", "WFSA_TIER2")}
    os.environ.update(WFSA_DENSE="0", WFSA_TIER2="0")
    try:
        dev = W.Device(0)
        dev.load_model(c.model.fsa)
        n = len(c.strings)
        dev.load_corpus(c.sym, c.off, np.full(n, 1.0 / n))
        assert dev.stats()["dense"] == 0 and dev.n_params == len(c.model.names)
        out = {}
        for wn, w in c.weightings.items():
            r = dict(best=dev.best_paths(w), kbest={k: dev.kbest_paths(w, k) for k in G.KS},
                     sample={m: dev.sample_paths(w, m, seed=G.SAMPLE_SEED) for m in NS}, counts=dev.posterior_counts(w),
                     plain=dev.byte_marginals(w), marg=dev.byte_marginals(w, decode=True))
            r["again"] = dict(best=dev.best_paths(w), kbest=dev.kbest_paths(w, 16), sample=dev.sample_paths(w, 64, seed=G.SAMPLE_SEED),
                              counts=dev.posterior_counts(w), marg=dev.byte_marginals(w, decode=True))
            out[wn] = r
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    _RUNS[name] = (c, out)
    return _RUNS[name]


def _groups(c):
    """string -> its corpus indices"""
    where = collections.defaultdict(list)
    for i, s in enumerate(c.strings):
        where[s].append(i)
    return where


def _same(*pairs):
    return all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in pairs)


def _cap(r):
    return float(PR.cap(r.posterior["logq"], r.L))


CASES = list(G.CASES)


@pytest.mark.parametrize("name", CASES)
def test_best_paths_are_the_first_of_the_total_order(name):
    c, out = _run(name)
    for wn, res in out.items():
        logw, prow, pidx = res["best"]
        assert logw.shape == (len(c.strings),) and prow[0] == 0 and prow[-1] == len(pidx)
        assert _same(*zip(res["best"], res["again"]["best"])), (name, wn)
        for s, idx in _groups(c).items():
            r = c.ref(wn, s)
            i0 = idx[0]
            ids = tuple(int(v) for v in pidx[prow[i0]:prow[i0 + 1]])
            if not r.finite:
                assert logw[i0] == -math.inf and ids == (), (name, wn, s)
            else:
                want = r.paths[r.order[0]]
                assert ids == want.ids, (name, wn, s, [c.model.names[j] for j in ids], [c.model.names[j] for j in want.ids])
                assert abs(logw[i0] - want.lw) <= _tol(want.lw), (name, wn, s, logw[i0], want.lw)
                _note("best_paths", logw=abs(logw[i0] - want.lw) / max(1.0, abs(want.lw)))
            for i in idx[1:]:   # equal strings, equal bytes
                assert logw[i:i + 1].tobytes() == logw[i0:i0 + 1].tobytes() and \
                    pidx[prow[i]:prow[i + 1]].tobytes() == pidx[prow[i0]:prow[i0 + 1]].tobytes(), (name, wn, s, i)


def _kpaths(result, i):
    srow, logw, prow, pidx = result
    return [(logw[t:t + 1], pidx[prow[t]:prow[t + 1]]) for t in range(srow[i], srow[i + 1])]


@pytest.mark.parametrize("name", CASES)
def test_kbest_paths_are_the_total_order_path_for_path(name):
    c, out = _run(name)
    for wn, res in out.items():
        assert _same(*zip(res["kbest"][16], res["again"]["kbest"])), (name, wn)
        blogw, bprow, bpidx = res["best"]
        for s, idx in _groups(c).items():
            r = c.ref(wn, s)
            i0 = idx[0]
            full = _kpaths(res["kbest"][16], i0)
            for k in G.KS:
                got = _kpaths(res["kbest"][k], i0)
                m = min(k, len(r.finite))
                assert len(got) == m, (name, wn, s, k, len(got), m)
                for t, (lw, ids) in enumerate(got):
                    want = r.paths[r.order[t]]
                    assert tuple(int(v) for v in ids) == want.ids, \
                        (name, wn, s, k, t, [c.model.names[j] for j in ids], [c.model.names[j] for j in want.ids])
                    assert abs(lw[0] - want.lw) <= _tol(want.lw), (name, wn, s, k, t, lw[0], want.lw)
                    _note("kbest_paths", logw=abs(lw[0] - want.lw) / max(1.0, abs(want.lw)))
                    # the k = j result is the byte prefix of the k = 16 result
                    assert lw.tobytes() == full[t][0].tobytes() and ids.tobytes() == full[t][1].tobytes(), (name, wn, s, k, t)
                if k == 1:   # ... and k = 1 carries best_paths' bytes
                    if m:
                        assert got[0][0].tobytes() == blogw[i0:i0 + 1].tobytes() and \
                            got[0][1].tobytes() == bpidx[bprow[i0]:bprow[i0 + 1]].tobytes(), (name, wn, s)
                    else:
                        assert blogw[i0] == -math.inf
                for i in idx[1:]:
                    other = _kpaths(res["kbest"][k], i)
                    assert len(other) == m and all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
                                                   for a, b in zip(got, other)), (name, wn, s, k, i)


@pytest.mark.parametrize("name", CASES)
def test_every_sample_is_the_replayed_walk(name):
    c, out = _run(name)
    for wn, res in out.items():
        assert _same(*zip(res["sample"][64], res["again"]["sample"])), (name, wn)
        ksrow, klogw, _, _ = res["kbest"][16]
        for n in NS:
            srow, logw, prow, pidx, logq = res["sample"][n]
            assert srow[-1] == len(logw) and prow[-1] == len(pidx)
            for s, idx in _groups(c).items():
                r = c.ref(wn, s)
                idx = np.array(idx)
                if not r.finite:
                    assert (logq[idx] == -math.inf).all() and (srow[idx + 1] == srow[idx]).all(), (name, wn, s)
                    continue
                assert (srow[idx + 1] - srow[idx] == n).all(), (name, wn, s)
                exact = r.posterior["logq"]
                err = np.abs(logq[idx] - exact).max() / max(1.0, abs(exact))
                assert err <= 1e-11, (name, wn, s, logq[idx[0]], exact)
                _note("sample_paths", logq=err)
                assert (logq[idx].view(np.int64) == logq[idx[0]:idx[0] + 1].view(np.int64)).all()
                which, ok = r.replay(G.draws(G.SAMPLE_SEED, idx, n, r.L))
                assert ok.all()   # (the CPU test's statement: no sample is left out)
                # the expected ids of all the samples of all the string's instances, and the device's
                width = max(len(p.ids) for p in r.paths)
                pad = np.full((len(r.paths), width), -1, dtype=np.int64)
                for l, p in enumerate(r.paths):
                    pad[l, :len(p.ids)] = p.ids
                chosen = pad[which]
                want_ids = chosen[chosen >= 0]
                want_len = (chosen >= 0).sum(axis=1)
                t0 = srow[idx]
                rows = (t0[:, None] + np.arange(n)[None, :]).reshape(-1)   # the samples' path numbers
                got_len = prow[rows + 1] - prow[rows]
                bad = np.flatnonzero(got_len != want_len)
                assert len(bad) == 0, (name, wn, s, n, "instance", int(idx[bad[0] // n]), "sample", int(bad[0] % n))
                got_ids = np.concatenate([pidx[prow[t]:prow[t + n]] for t in t0]) if len(pidx) else np.zeros(0, dtype=np.int64)
                if not np.array_equal(got_ids, want_ids):   # (the lengths agree sample by sample)
                    first = int(np.repeat(np.arange(len(rows)), want_len)[np.flatnonzero(got_ids != want_ids)[0]])
                    raise AssertionError((name, wn, s, n, "instance", int(idx[first // n]), "sample", first % n,
                                          [c.model.names[j] for j in r.paths[which[first]].ids]))
                # the weight: the path's one sum, and kbest_paths' bytes where the path is among the 16 best
                want_lw = np.array([p.lw for p in r.paths])[which]
                assert (np.abs(logw[rows] - want_lw) <= 1e-12 * np.maximum(1.0, np.abs(want_lw))).all(), (name, wn, s)
                rank = np.full(len(r.paths), -1)
                rank[r.order[:16]] = np.arange(min(16, len(r.order)))
                rk = rank[which]
                kt = np.repeat(ksrow[idx], n) + rk
                listed = rk >= 0
                assert (logw[rows][listed].view(np.int64) == klogw[kt[listed]].view(np.int64)).all(), (name, wn, s)
                if n == 64:   # the first sample of the n = 64 result is the n = 1 result
                    s1, l1, p1, i1, _ = res["sample"][1]
                    a = s1[idx[0]]
                    assert l1[a:a + 1].tobytes() == logw[t0[0]:t0[0] + 1].tobytes() and \
                        i1[p1[a]:p1[a + 1]].tobytes() == pidx[prow[t0[0]]:prow[t0[0] + 1]].tobytes(), (name, wn, s)


@pytest.mark.parametrize("name", CASES)
def test_posterior_counts_are_the_exact_posteriors(name):
    c, out = _run(name)
    for wn, res in out.items():
        crow, cidx, cval, logq, ent = res["counts"]
        assert _same(*zip(res["counts"], res["again"]["counts"])), (name, wn)   # a second call: the same bytes
        assert logq.tobytes() == res["sample"][64][4].tobytes() == res["sample"][1][4].tobytes(), (name, wn)
        assert crow[0] == 0 and crow[-1] == len(cidx) == len(cval)
        for s, idx in _groups(c).items():
            r = c.ref(wn, s)
            p = r.posterior
            i0 = idx[0]
            ids, val = cidx[crow[i0]:crow[i0 + 1]], cval[crow[i0]:crow[i0 + 1]]
            if not r.finite:
                assert len(ids) == 0 and logq[i0] == -math.inf and np.isnan(ent[i0]), (name, wn, s)
            else:
                want = sorted(j for j, v in p["counts"].items() if v > 0.0)
                assert [int(j) for j in ids] == want, (name, wn, s)   # exactly the parameters of positive count, ascending
                exact = np.array([p["counts"][j] for j in want])
                cap = _cap(r)
                if name in EXACT:
                    assert val.tobytes() == exact.tobytes() and ent[i0] == 0.0, (name, wn, s, val, ent[i0])
                e_c, e_h = np.abs(val - exact).max(), abs(ent[i0] - p["entropy"])
                assert e_c <= cap and e_h <= cap, (name, wn, s, e_c, e_h, cap)
                _note("posterior_counts", count=e_c, entropy=e_h, count_over_cap=e_c / cap, entropy_over_cap=e_h / cap)
            for i in idx[1:]:
                assert cidx[crow[i]:crow[i + 1]].tobytes() == ids.tobytes() and cval[crow[i]:crow[i + 1]].tobytes() == val.tobytes() and \
                    ent[i:i + 1].tobytes() == ent[i0:i0 + 1].tobytes() and logq[i:i + 1].tobytes() == logq[i0:i0 + 1].tobytes(), (name, wn, s, i)
    if name == "seam63":   # the row scan across its rounds of 64 ids
        case, wn, s = G.ids65()
        i0 = c.strings.index(s)
        crow, cidx = out[wn]["counts"][:2]
        assert case is c and {63, 64, 65} <= set(int(j) for j in cidx[crow[i0]:crow[i0 + 1]])


@pytest.mark.parametrize("name", CASES)
def test_byte_marginals_and_the_mea_decode(name):
    c, out = _run(name)
    for wn, res in out.items():
        mrow, midx, mval, boundary, logq, score, plw, prow, pidx = res["marg"]
        assert _same(*zip(res["marg"], res["again"]["marg"])) and _same(*zip(res["plain"], res["marg"][:5])), (name, wn)
        assert logq.tobytes() == res["counts"][3].tobytes(), (name, wn)
        assert mrow.shape == (int(c.off[-1]) + 1,) and mrow[0] == 0 and mrow[-1] == len(midx) == len(mval)
        kb = res["kbest"][16]
        for s, idx in _groups(c).items():
            r = c.ref(wn, s)
            p = r.posterior
            i0, L = idx[0], r.L
            b0 = int(c.off[i0])
            ids = pidx[prow[i0]:prow[i0 + 1]]
            if not r.finite:
                assert mrow[b0 + L] == mrow[b0] and np.isnan(boundary[b0:b0 + L]).all() and np.isnan(score[i0]) and \
                    plw[i0] == -math.inf and len(ids) == 0, (name, wn, s)
            else:
                cap = _cap(r)
                device_mass = []
                for i in range(L):
                    a, b = mrow[b0 + i], mrow[b0 + i + 1]
                    got = {int(u): float(v) for u, v in zip(midx[a:b], mval[a:b])}
                    device_mass.append(got)
                    want = p["mass"][i]
                    assert list(midx[a:b]) == sorted(u for u, v in want.items() if v > 0.0), (name, wn, s, i)   # exactly the states of mass
                    e_m = max(abs(got[u] - want[u]) for u in got)
                    e_s = abs(math.fsum(got.values()) - 1.0)
                    e_b = abs(boundary[b0 + i] - p["boundary"][i])
                    assert e_m <= cap and e_s <= cap and e_b <= cap, (name, wn, s, i, e_m, e_s, e_b, cap)
                    if name in EXACT:
                        assert list(got.values()) == [1.0] and boundary[b0 + i] == 1.0, (name, wn, s, i)
                    _note("byte_marginals", mass=e_m, boundary=e_b, sum=e_s, mass_over_cap=e_m / cap)
                # the MEA path: the first in marginals.hpp's order under the masses the device stored
                l, want_score = r.mea(device_mass)
                assert tuple(int(v) for v in ids) == r.paths[l].ids, \
                    (name, wn, s, [c.model.names[j] for j in ids], [c.model.names[j] for j in r.paths[l].ids])
                assert abs(plw[i0] - r.paths[l].lw) <= _tol(r.paths[l].lw)
                for lw_t, ids_t in _kpaths(kb, i0):   # its weight: kbest_paths' bytes where listed
                    if ids_t.tobytes() == ids.tobytes():
                        assert lw_t.tobytes() == plw[i0:i0 + 1].tobytes(), (name, wn, s)
                e_sc = abs(score[i0] - r.mea_score(l, p["mass"]))
                assert e_sc <= L * cap and score[i0] == want_score, (name, wn, s, score[i0], want_score, r.mea_score(l, p["mass"]))
                if L:
                    _note("byte_marginals", score_over_L_cap=e_sc / (L * cap))
            for i in idx[1:]:
                b1 = int(c.off[i])
                assert mrow[b1 + L] - mrow[b1] == mrow[b0 + L] - mrow[b0] and \
                    midx[mrow[b1]:mrow[b1 + L]].tobytes() == midx[mrow[b0]:mrow[b0 + L]].tobytes() and \
                    mval[mrow[b1]:mrow[b1 + L]].tobytes() == mval[mrow[b0]:mrow[b0 + L]].tobytes() and \
                    boundary[b1:b1 + L].tobytes() == boundary[b0:b0 + L].tobytes() and \
                    score[i:i + 1].tobytes() == score[i0:i0 + 1].tobytes() and plw[i:i + 1].tobytes() == plw[i0:i0 + 1].tobytes() and \
                    pidx[prow[i]:prow[i + 1]].tobytes() == ids.tobytes(), (name, wn, s, i)


def test_the_empty_string_on_every_walker():
    """^ -> $ beside ^ -> H: the empty string, alone in its corpus and between
    others, has one path of one end edge, log q equal to that edge's weight,
    entropy 0, one count and no marginal rows"""
    for name in ("empty_alone", "empty"):
        c, out = _run(name)
        j = c.model.pid[(G.START, "T", G.END)]
        for wn, res in out.items():
            w = c.weightings[wn][j]
            for i in _groups(c)[b""]:
                logw, prow, pidx = res["best"]
                assert list(pidx[prow[i]:prow[i + 1]]) == [j] and logw[i] == w
                for k in G.KS:
                    got = _kpaths(res["kbest"][k], i)
                    assert len(got) == 1 and list(got[0][1]) == [j] and got[0][0][0] == w
                srow, slogw, sprow, spidx, slogq = res["sample"][64]
                assert srow[i + 1] - srow[i] == 64 and (slogw[srow[i]:srow[i + 1]] == w).all() and slogq[i] == w
                assert (spidx[sprow[srow[i]]:sprow[srow[i + 1]]] == j).all() and sprow[srow[i + 1]] - sprow[srow[i]] == 64
                crow, cidx, cval, logq, ent = res["counts"]
                assert list(cidx[crow[i]:crow[i + 1]]) == [j] and list(cval[crow[i]:crow[i + 1]]) == [1.0] and logq[i] == w and ent[i] == 0.0
                mrow, midx, mval, boundary, mlogq, score, plw, mprow, mpidx = res["marg"]
                assert mrow[c.off[i]] == mrow[c.off[i + 1]] and mlogq[i] == w and score[i] == 0.0 and plw[i] == w
                assert list(mpidx[mprow[i]:mprow[i + 1]]) == [j]
        if name == "empty_alone":
            assert len(res["marg"][1]) == 0 and len(res["marg"][3]) == 0 and list(res["marg"][0]) == [0]
