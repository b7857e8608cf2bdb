"""Path matrices large enough for several blocks of every matrix-file-mode
kernel (256 threads each), generated directly -- load_paths needs no
automaton --, and the SpMV chain over them in a chosen precision
(test_matrix_blocks_reference.py, test_gpu_matrix_blocks.py) -- test
infrastructure.

16,684 strings are 65 full blocks of mp_string_kernel and a 44-string tail:
66 partials, two more than one round of mp_rmin_kernel's 64 lanes."""
import functools

import numpy as np

N_STRINGS = 16684
N_PARAMS = 700
HEAVY = {100: 823, 2000: 300, 5000: 257, 9000: 256, 12000: 65, N_STRINGS - 1: 64}   # string -> paths
# Two strings with identical path rows tie exactly for the global rmin; the
# lower path index has to win wherever the two meet.  name -> (string a,
# string b > a, which of them holds the lower path index).  Each is placed so
# that a min_pair without its tie clause (`v2 == v && i2 < i`), which keeps
# the value it already holds, returns the HIGHER index (simulate_rmin shows it
# for every one, test_matrix_blocks_reference.py):
# - a butterfly `for o = 32 .. 1: min_pair(own, lane ^ o)` brings lane L's
#   value to lane 0 at the step o = lowest set bit of L, so of two tying lanes
#   the one with the larger lowest set bit is the value lane 0 already holds;
# - thread 0 of a block folds waves 1 .. 3 into wave 0's value in order;
# - lane k of mp_rmin_kernel folds partial k + 64 into partial k.
PLANTS = {
    "blocks4+61": (4 * 256 + 17, 61 * 256 + 200, "b"),      # across blocks, the later string wins: lane 4 reaches lane 0 first
    "blocks3+60": (3 * 256 + 17, 60 * 256 + 200, "a"),      # across blocks, the earlier string wins: lane 60 reaches lane 0 first
    "blocks1+65": (1 * 256 + 5, 65 * 256 + 10, "b"),        # the strided loop past 64 partials (block 65 is the 44-string tail)
    "waves0+2": (7 * 256 + 9, 7 * 256 + 2 * 64 + 30, "b"),  # one block, waves 0 and 2: thread 0's fold over sv/si
    "lanes8+13": (9 * 256 + 64 + 8, 9 * 256 + 64 + 13, "b"),  # one wave, lanes 8 and 13: the shuffle butterfly
}
PLANT = PLANTS["blocks4+61"][:2]


def _rows(rng, n_paths, prob):
    """CSR rows of 1 .. 40 entries, counts 1 .. 3, columns by popularity
    (a column may repeat within a row: its entries add up)"""
    k = rng.integers(1, 41, size=n_paths)
    prow = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
    pcol = rng.choice(len(prob), size=int(prow[-1]), p=prob).astype(np.int32)
    pdata = rng.integers(1, 4, size=int(prow[-1])).astype(np.float64)
    return prow, pcol, pdata


def _permute_rows(prow, pcol, pdata, mcol):
    """P row mcol[k] <- row k"""
    src = np.argsort(mcol)
    cnt = np.diff(prow)[src]
    idx = np.repeat(prow[:-1][src], cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    return np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64), pcol[idx], pdata[idx]


@functools.lru_cache(maxsize=None)
def synthetic(single=False, seed=5, plant="blocks4+61"):
    """dict(n, prow, pcol, pdata, mrow, mcol, p, plant).  single: every string
    has exactly one path (no ambiguous string anywhere); plant: the PLANTS
    entry (the rest of the corpus is drawn the same for every one)"""
    sa, sb, lower = PLANTS[plant]
    assert sa < sb and sa not in HEAVY and sb not in HEAVY
    rng = np.random.default_rng(seed)
    S, n = N_STRINGS, N_PARAMS
    prob = 1.0 / (np.arange(n) + 3.0)          # heavy tail: the busiest column draws ~6 % of the entries
    prob = (prob / prob.sum())[rng.permutation(n)]
    cnt = rng.integers(1, 9, size=S)
    cnt[rng.random(S) < 0.3] = 1
    for s, c in HEAVY.items():
        cnt[s] = c
    cnt[[sa, sb]] = 2
    if single:
        cnt[:] = 1
    mrow = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    n_paths = int(mrow[-1])
    prow, pcol, pdata = _rows(rng, n_paths, prob)
    mcol = rng.permutation(n_paths).astype(np.int64)
    if not single:
        # the planted pair: a one-entry path and a path of 40 entries of count
        # 6 (twice what any other path can weigh, so its relative probability
        # is the smallest at any weights drawn), the same rows in both strings
        rows = [(rng.choice(n, size=1, p=prob).astype(np.int32), np.ones(1)),
                (rng.choice(n, size=40, p=prob).astype(np.int32), np.full(40, 6.0))]
        lens = np.diff(prow)
        for s in (sa, sb):
            for q, (c, d) in enumerate(rows):
                lens[mrow[s] + q] = len(c)
        new_prow = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        new_pcol = np.zeros(int(new_prow[-1]), dtype=np.int32)
        new_pdata = np.zeros(int(new_prow[-1]))
        planted = {int(mrow[s] + q): rows[q] for s in (sa, sb) for q in range(2)}
        keep = np.ones(n_paths, dtype=bool)
        keep[list(planted)] = False
        old = np.repeat(keep, np.diff(prow))
        new = np.repeat(keep, lens)
        new_pcol[new], new_pdata[new] = pcol[old], pdata[old]
        for l, (c, d) in planted.items():
            new_pcol[new_prow[l]:new_prow[l + 1]] = c
            new_pdata[new_prow[l]:new_prow[l + 1]] = d
        prow, pcol, pdata = new_prow, new_pcol, new_pdata
        # the improbable path of string `lower` gets the lower path index
        a, b = int(mrow[sa] + 1), int(mrow[sb] + 1)
        if (mcol[b] > mcol[a]) == (lower == "b"):
            mcol[a], mcol[b] = mcol[b], mcol[a]
    prow, pcol, pdata = _permute_rows(prow, pcol, pdata, mcol)
    p = rng.random(S) + 0.5
    return dict(n=n, prow=prow, pcol=pcol, pdata=pdata, mrow=mrow, mcol=mcol, p=p / p.sum(), plant=(sa, sb, lower))


def chain(m, x, dtype=np.longdouble, reverse=False):
    """(ll, logq, grad, rpp) of the reference's SpMV chain in `dtype`:
    lw = P x, a log-sum-exp per string, rpp, grad = -P^T (p . rpp); reverse:
    every sum taken in the opposite order"""
    prow, pcol, pdata, mrow, mcol = m["prow"], m["pcol"], m["pdata"], m["mrow"], m["mcol"]
    n_paths, S = len(prow) - 1, len(mrow) - 1
    x = np.asarray(x, dtype=dtype)
    p = np.asarray(m["p"], dtype=dtype)

    def segsum(v, ptr):     # sums of v[ptr[i]:ptr[i + 1]], no segment empty
        if reverse:
            return np.add.reduceat(v[::-1], (len(v) - ptr[1:])[::-1])[::-1]
        return np.add.reduceat(v, ptr[:-1])

    assert (np.diff(prow) > 0).all() and (np.diff(mrow) > 0).all()
    lw = segsum(pdata.astype(dtype) * x[pcol], prow)
    lm = lw[mcol]
    per = np.diff(mrow)
    mx = np.maximum.reduceat(lm, mrow[:-1])
    e = np.exp(lm - np.repeat(mx, per))
    q = segsum(e, mrow)
    logq = mx + np.log(q)
    r = e / np.repeat(q, per)
    rpp = np.zeros(n_paths, dtype=dtype)
    coef = np.zeros(n_paths, dtype=dtype)
    rpp[mcol] = r
    coef[mcol] = np.repeat(p, per) * r
    order = np.argsort(pcol, kind="stable")
    tptr = np.concatenate([[0], np.cumsum(np.bincount(pcol, minlength=m["n"]))])
    assert (np.diff(tptr) > 0).all()
    path_of = np.repeat(np.arange(n_paths), np.diff(prow))
    grad = -segsum((pdata.astype(dtype) * coef[path_of])[order], tptr)
    ll = (p * logq)[::-1].sum() if reverse else (p * logq).sum()
    return ll, logq, grad, rpp


def rmin_of(m, rpp):
    """(smallest relative path probability of an ambiguous string, its path
    index -- the lowest on a tie); (0.0, -1) when no string is ambiguous"""
    amb = np.zeros(len(rpp), dtype=bool)
    amb[m["mcol"]] = np.repeat(np.diff(m["mrow"]) > 1, np.diff(m["mrow"]))
    if not amb.any():
        return 0.0, -1
    i = int(np.argmin(np.where(amb, rpp, np.inf)))
    return rpp[i], i


def simulate_rmin(m, rpp, tie_rule=True):
    """matrix_path.hip's rmin reduction in its own order, on the CPU: a
    string per lane folds its paths in M's order, the 64 lanes of a wave a
    xor butterfly (32 .. 1), thread 0 the block's waves 1 .. 3 into wave 0's
    value, then mp_rmin_kernel's 64 lanes the partials k, k + 64, ... and a
    butterfly again.  tie_rule=False: min_pair without `v2 == v && i2 < i`.
    Returns lane 0's (value, path index)"""
    mrow, mcol = m["mrow"], m["mcol"]
    S = len(mrow) - 1

    def take(v, i, v2, i2):
        t = (v2 < v) | ((v2 == v) & (i2 < i) if tie_rule else False)
        return np.where(t, v2, v), np.where(t, i2, i)

    def butterfly(v, i):      # over the last axis, 64 lanes
        lanes = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            v, i = take(v, i, v[..., lanes ^ o], i[..., lanes ^ o])
        return v[..., 0], i[..., 0]

    nb = (S + 255) // 256
    v = np.full(nb * 256, np.inf)
    i = np.full(nb * 256, -1.0)
    r = np.asarray(rpp, dtype=np.float64)
    for s in np.flatnonzero(np.diff(mrow) > 1):
        for k in range(mrow[s], mrow[s + 1]):
            v[s], i[s] = take(v[s], i[s], r[mcol[k]], float(mcol[k]))
    wv, wi = butterfly(v.reshape(nb, 4, 64), i.reshape(nb, 4, 64))
    pv, pi = wv[:, 0], wi[:, 0]
    for k in (1, 2, 3):
        pv, pi = take(pv, pi, wv[:, k], wi[:, k])
    lv, li = np.full(64, np.inf), np.full(64, -1.0)
    for k in range(nb):
        lv[k % 64], li[k % 64] = take(lv[k % 64], li[k % 64], pv[k], pi[k])
    fv, fi = butterfly(lv, li)
    return (float(fv), int(fi)) if fi >= 0 else (0.0, -1)


N20 = dict(n_states=20, degree=4, vocab=6, emissions=2, n_strings=300, max_len=12, seed=3)
N20_ETA = 0.05      # the Hessian epochs' step on this family (test_matrix_blocks_reference.py says why)


@functools.lru_cache(maxsize=None)
def n20():
    """(oracle, dense restatement) of the N20 family: 59,380 paths over 300 strings"""
    import wfsa_amd as W
    from oracle import Oracle
    from oracle.hessian import HessianOracle
    syn = W.Synthetic(**N20)
    sym, off, wt = syn.corpus()
    o = Oracle.from_arrays(syn.wfsa_text, sym, off, wt)
    assert o.info["n_paths"] == 59380 and o.info["n_strings"] == 300
    return o, HessianOracle(o)


def isolated_minimum(rpp):
    """whether the smallest relative path probability stands 1e-9 (relative) clear of the next"""
    lo = np.partition(rpp, 1)[:2]
    return bool(lo[1] > lo[0] * (1 + 1e-9))


def draws(m, seed=11, k=3):
    rng = np.random.default_rng(seed)
    return [rng.normal(-1.0, 0.5, size=m["n"]) for _ in range(k)]
