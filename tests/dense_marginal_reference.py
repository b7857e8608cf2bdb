"""Numpy restatement of the dense path's byte marginals and MEA decode
(wfsa_dev_dense_byte_marginals, include/wfsa_dev.h), per string in float64.

The masses do NOT share the device's arithmetic: the device scales every
alpha and beta row by its sum and multiplies exp(la + lb - log q) back in;
here log alpha and log beta are kept as logarithms over
dense_decode_reference.Tables -- each step log(exp(x - max x) . exp(lA)) +
max x -- and mass = exp(log alpha + log beta - log q).

mea_replay restates the decode operation for operation: the eligibility
masks of the log tables (an entry above -inf), D = (max over the eligible
sources) + reward with the max first and one add, np.argmax for the lowest
state, a -inf candidate never taken, the ids and path_logw as
dense_decode_reference.decode forms them.  Fed with the device's own stored
masses it must return the device's bytes -- test infrastructure."""
import numpy as np

from dense_decode_reference import Tables

CAP = 3e-11   # the project's cap on a mass: CAP * max(1, |log q|) * (L + 1)


def cap(logq, L):
    return CAP * max(1.0, abs(float(logq))) * (L + 1)


def state_ids(fsa):
    """interior index -> Fsa state id (wfsa_model_desc numbering), ascending"""
    d = fsa.desc()
    return np.array([s for s in range(d.n_states) if s != d.start and s != d.end], dtype=np.int32)


def _lse_rows(x, M):
    """log(exp(x) . M) per column, M >= 0: the greatest term taken out first"""
    m = x.max()
    if not m > -np.inf:
        return np.full(M.shape[1], -np.inf)
    with np.errstate(divide="ignore", under="ignore"):
        return np.log(np.exp(x - m).dot(M)) + m


def marginals(tab, s, A=None):
    """(log q, mass [L][n]) of one string (bytes as integers) in the log
    domain; mass None when log q is -inf; the empty string: (lse, [0][n])"""
    s = np.asarray(s, dtype=np.int64)
    L = len(s)
    if L == 0:
        return (float(tab.lse) if tab.pse != -2 else -np.inf), np.zeros((0, tab.n))
    with np.errstate(under="ignore"):
        A = np.exp(tab.lA) if A is None else A
    la, lb = np.empty((L, tab.n)), np.empty((L, tab.n))
    la[0] = tab.l0 + tab.lE[:, s[0]]
    for j in range(1, L):
        la[j] = _lse_rows(la[j - 1], A) + tab.lE[:, s[j]]
    lb[L - 1] = tab.lend
    for j in range(L - 2, -1, -1):
        lb[j] = _lse_rows(tab.lE[:, s[j + 1]] + lb[j + 1], A.T)
    fin = la[L - 1] + tab.lend
    m = fin.max()
    if not m > -np.inf:
        return -np.inf, None
    logq = float(np.log(np.exp(fin - m).sum()) + m)
    with np.errstate(under="ignore", invalid="ignore"):
        t = la + lb   # (-inf + -inf is -inf; never +inf here)
        mass = np.where(t > -np.inf, np.exp(t - logq), 0.0)
    return logq, mass


def stored_row(gamma):
    """the listing rule on one byte's masses over the interior states: the
    stored value is min(gamma, 1.0), a state is listed when that is > 0 --
    (interior indices ascending, values)"""
    v = np.minimum(np.asarray(gamma, dtype=np.float64), 1.0)
    idx = np.flatnonzero(v > 0.0)
    return idx.astype(np.int32), v[idx]


def mea_replay(tab, s, mass):
    """the decode of one string at the stored masses mass [L][n] (0.0 for an
    unlisted state; None: the string has log q = -inf and owns nothing):
    (states, ids in path order, score, path_logw); no path: ([], [], NaN, -inf)"""
    none = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int32), np.nan, -np.inf)
    s = np.asarray(s, dtype=np.int64)
    L = len(s)
    if mass is None:
        return none
    if L == 0:
        if tab.pse == -2:
            return none
        total = 0.0 + tab.edge_lw(tab.pse)
        if not total > -np.inf:
            return none
        return none[0], np.array([tab.pse] if tab.pse >= 0 else [], dtype=np.int32), 0.0, total
    elA, elE, el0, elend = tab.lA > -np.inf, tab.lE > -np.inf, tab.l0 > -np.inf, tab.lend > -np.inf
    D = np.empty((L, tab.n))
    D[0] = np.where(el0 & elE[:, s[0]], 0.0 + mass[0], -np.inf)
    for j in range(1, L):
        best = np.max(np.where(elA, D[j - 1][:, None], -np.inf), axis=0)   # the max first
        D[j] = np.where(elE[:, s[j]], best + mass[j], -np.inf)             # then one add
    v = np.where(elend, D[L - 1], -np.inf)
    if not v.max() > -np.inf:
        return none
    cur = int(np.argmax(v))
    score = float(v[cur])
    states = [cur]
    for j in range(L - 1, 0, -1):
        v = np.where(elA[:, cur], D[j - 1], -np.inf)
        assert v.max() > -np.inf
        cur = int(np.argmax(v))
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
    return np.array(states, dtype=np.int64), np.array(ids, dtype=np.int32), score, total


def path_score(mass, states):
    """the MEA score of a path under masses [L][n]: one left-to-right sum"""
    t = 0.0
    for j, T in enumerate(states):
        t = t + mass[j, T] if j else 0.0 + mass[j, T]
    return t


def path_states(tab, s, ids):
    """the interior states of the path with parameter ids `ids` (path order,
    single-member groups without an id) over the bytes s: a depth-first match
    of the ids against the tables, None if no accepting path spells them"""
    s = np.asarray(s, dtype=np.int64)
    ids = [int(i) for i in ids]
    L = len(s)

    def eat(k, *params):
        for p in params:
            if p == -2:
                return -1
            if p >= 0:
                if k >= len(ids) or ids[k] != p:
                    return -1
                k += 1
        return k

    dead = set()   # (byte, state before it, ids eaten) from which no match exists

    def walk(j, prev, k):
        if j == L:
            return [] if eat(k, tab.pend[prev]) == len(ids) else None
        if (j, prev, k) in dead:
            return None
        for T in range(tab.n):
            k2 = eat(k, tab.p0[T] if j == 0 else tab.pA[prev, T], tab.pE[T, s[j]])
            if k2 >= 0:
                rest = walk(j + 1, T, k2)
                if rest is not None:
                    return [T] + rest
        dead.add((j, prev, k))
        return None

    return walk(0, -1, 0) if L else []


def corpus(fsa, w, sym, off):
    """every string: (logq [S], masses: a list of [L][n] arrays or None)"""
    tab = Tables(fsa, w)
    with np.errstate(under="ignore"):
        A = np.exp(tab.lA)
    S = len(off) - 1
    logq, masses = np.empty(S), []
    for i in range(S):
        logq[i], m = marginals(tab, sym[off[i]:off[i + 1]], A)
        masses.append(m)
    return logq, masses


_MEMO = {}


def clear_caches():
    """drop the memoised cases (they hold Fsa handles: not to be left for interpreter exit)"""
    _MEMO.clear()


def expected(name):
    """(fsa, w, sym, off, p, Tables, logq, masses) of a dense_sample_reference
    case ("without_a_path" too), computed once and left unchanged"""
    if name not in _MEMO:
        import dense_sample_reference as D
        fsa, w, sym, off, p = D.without_a_path_case() if name == "without_a_path" else D.case(name)
        logq, masses = corpus(fsa, w, sym, off)
        logq.setflags(write=False)
        for m in masses:
            if m is not None:
                m.setflags(write=False)
        _MEMO[name] = (fsa, w, sym, off, p, Tables(fsa, w), logq, masses)
    return _MEMO[name]
