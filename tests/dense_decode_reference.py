"""Numpy restatement of the dense path's Viterbi decode
(wfsa_dev_dense_best_paths, include/wfsa_dev.h), per string and operation for
operation: log tables from w directly, D = max_S(D[S] + lA[S][T]) + lE[T]
(the max first, then one add), the end state by D + lend, every predecessor
by D_prev + lA[:, T], np.argmax for the lowest index on ties, a -inf
candidate never chosen, and best_logw as the decoders form it (an edge's
weight the left-to-right sum, from 0.0, of its present parameters; the path's
the left-to-right sum, from 0.0, of its edges).  For every decision on the
returned path it also gives the gap between the best and the second-best
distinct candidate value, and counts the candidates that tie with the best
exactly -- test infrastructure, and the cases the GPU tests
compare byte for byte with the trellis decode (BYTE_CASES)."""
import ctypes as C
import functools

import numpy as np

# (model, seed of the weight draw) of the GPU tests' byte-for-byte comparisons
# with the trellis decode; test_dense_decode_reference.py checks on the CPU
# that every decision on every returned path is wider than 1e-9 and meets no
# exact tie for each (dense16 at draw 2 fails that: two of its best paths run
# through the same edges in another order, sums equal to the bit here and one
# ulp apart where the trellis decode rounds D + (lA + lE))
BYTE_CASES = {
    "dense16": (dict(n_states=16, degree=1, vocab=6, emissions=2, dense=True, n_strings=500, max_len=9, seed=3), 1),
    "auto128": (dict(n_states=128, degree=1, vocab=4, emissions=4, dense=True, n_strings=50, max_len=8, seed=1), 4),
}


@functools.lru_cache(maxsize=None)
def synthetic(name):
    """(wfsa text, sym, off, wt) of a BYTE_CASES model, built once"""
    import wfsa_amd as W
    syn = W.Synthetic(**BYTE_CASES[name][0])
    return (syn.wfsa_text,) + tuple(syn.corpus())


def case_weights(name, n_params):
    return np.random.default_rng(BYTE_CASES[name][1]).normal(-1.0, 0.5, size=n_params)


class Tables:
    """log tables over the interior states (state order, ^ and $ left out, as
    the device numbers them): lA[S][T], lE[T][byte], l0[T], lend[T], lse
    (^ -> $), and the parameter of each entry (>= 0 an Fsa parameter, -1 a
    single-member group, -2 no such edge)"""

    def __init__(self, fsa, w):
        d = fsa.desc()
        ns = d.n_states

        def arr(ptr, n, ct):
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ct)), shape=(n,)).copy()

        tr_ptr = arr(d.tr_ptr, ns + 1, C.c_int32)
        n_tr = int(tr_ptr[-1])
        tr_dst = arr(d.tr_dst, n_tr, C.c_int32)
        tr_par = arr(d.tr_param, n_tr, C.c_int32)
        em_ptr = arr(d.em_ptr, ns + 1, C.c_int32)
        n_em = int(em_ptr[-1])
        em_off = arr(d.em_off, n_em, C.c_int64)
        em_len = arr(d.em_len, n_em, C.c_int32)
        em_par = arr(d.em_param, n_em, C.c_int32)
        em_bytes = arr(d.em_bytes, int((em_off + em_len).max()) if n_em else 1, C.c_uint8)
        w = np.asarray(w, dtype=np.float64)
        self.w = w
        interior = np.array([s for s in range(ns) if s != d.start and s != d.end])
        n = len(interior)
        idx = np.full(ns, -1)
        idx[interior] = np.arange(n)
        src = np.repeat(np.arange(ns), np.diff(tr_ptr))
        full_p = np.full((ns, ns), -2)
        full_p[src, tr_dst] = np.where(tr_par >= 0, tr_par, -1)
        self.pA = full_p[np.ix_(interior, interior)]
        self.p0 = full_p[d.start, interior]
        self.pend = full_p[interior, d.end]
        self.pse = int(full_p[d.start, d.end])
        esrc = np.repeat(np.arange(ns), np.diff(em_ptr))
        own = idx[esrc] >= 0   # (^ and $ emit nothing that counts)
        assert (em_len[own] == 1).all()
        self.pE = np.full((n, 256), -2)
        self.pE[idx[esrc[own]], em_bytes[em_off[own]]] = np.where(em_par[own] >= 0, em_par[own], -1)
        self.n = n
        self.lA, self.lE, self.l0, self.lend = (self._log(p) for p in (self.pA, self.pE, self.p0, self.pend))
        self.lse = float(self._log(np.array([self.pse]))[0])

    def _log(self, par):
        return np.where(par >= 0, self.w[np.maximum(par, 0)], np.where(par == -1, 0.0, -np.inf))

    def edge_lw(self, *params):
        """the decoders' weight of one edge: its present parameters, left to right from 0.0"""
        t = 0.0
        for p in params:
            if p >= 0:
                t += self.w[p]
        return t


def _decide(v):
    """(arg, gap, ties) of one decision: the lowest index of the maximum, the
    distance to the second-best distinct value (inf: none) and how many other
    candidates hold the maximum exactly; arg -1 when the maximum is -inf"""
    best = v.max()
    if not best > -np.inf:
        return -1, np.inf, 0
    rest = v[v < best]
    gap = best - rest.max() if rest.size else np.inf
    return int(np.argmax(v)), float(gap), int((v == best).sum()) - 1


def decode(tab, s):
    """one string (bytes as integers): (best_logw, ids in path order, smallest
    on-path gap, exact ties met on the path)"""
    none = (-np.inf, np.zeros(0, dtype=np.int32), np.inf, 0)
    L = len(s)
    if L == 0:
        if tab.pse == -2:
            return none
        total = 0.0 + tab.edge_lw(tab.pse)
        if not total > -np.inf:
            return none
        return total, np.array([tab.pse] if tab.pse >= 0 else [], dtype=np.int32), np.inf, 0
    D = np.empty((L, tab.n))
    D[0] = tab.l0 + tab.lE[:, s[0]]
    for j in range(1, L):
        D[j] = np.max(D[j - 1][:, None] + tab.lA, axis=0) + tab.lE[:, s[j]]
    cur, gap, ties = _decide(D[L - 1] + tab.lend)
    if cur < 0:
        return none
    states = [cur]
    for j in range(L - 1, 0, -1):
        cur, g, t = _decide(D[j - 1] + tab.lA[:, cur])
        assert cur >= 0
        gap, ties = min(gap, g), ties + t
        states.append(cur)
    states.reverse()
    ids, total, prev = [], 0.0, -1
    for j, T in enumerate(states):
        pt = tab.p0[T] if j == 0 else tab.pA[prev, T]
        pe = tab.pE[T, s[j]]
        total += tab.edge_lw(pt, pe)
        ids += [p for p in (pt, pe) if p >= 0]
        prev = T
    total += tab.edge_lw(tab.pend[prev])
    if tab.pend[prev] >= 0:
        ids.append(tab.pend[prev])
    return total, np.array(ids, dtype=np.int32), gap, ties


def decode_corpus(fsa, w, sym, off):
    """every string: (logw [S], prow [S + 1], pidx, gap [S], ties [S]) in best_paths' layout"""
    tab = Tables(fsa, w)
    S = len(off) - 1
    logw, gaps, ties, prow, parts = np.empty(S), np.empty(S), np.zeros(S, dtype=np.int64), np.zeros(S + 1, dtype=np.int64), []
    for i in range(S):
        logw[i], ids, gaps[i], ties[i] = decode(tab, sym[off[i]:off[i + 1]])
        parts.append(ids)
        prow[i + 1] = prow[i] + len(ids)
    pidx = np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, dtype=np.int32)
    return logw, prow, pidx, gaps, ties
