"""The exact second-order term H_f from enumerated paths, in long double, and
the cases the H_f tests share (test_hf_reference.py, test_gpu_hf_exact.py) --
test infrastructure.

    H[j,k] = sum_s p_s (E_s[c_j c_k] - E_s[c_j] E_s[c_k])
    B[j,k] = sum_s p_s (E_s[c_j c_k] + E_s[c_j] E_s[c_k])

over the ambiguous strings s and their equivocal parameters V_s (the columns
of P whose count is not the same on all of the string's paths; AssembleH's
per-string set), under the string's relative path probabilities at x.  B is
the sum H would be without cancellation: B > 0 exactly on the union of
V_s x V_s (every equivocal parameter has a positive expected count), so it is
both the pattern and the scale every device value is held to:

    |D - H| <= TOL * B  entrywise, and D == 0 wherever B == 0.

oracle/hessian.py's HessianOracle.hf is the float64 restatement of the same
sum with the other sign (-Cov)."""
import functools

import numpy as np

TOL = 1e-12

LD = np.longdouble


def equivocal_sets(P, mrow):
    """[(string, V_s)] for every string with more than one path and a non-empty V_s"""
    out = []
    for s in range(len(mrow) - 1):
        a, b = int(mrow[s]), int(mrow[s + 1])
        if b - a < 2:
            continue
        rows = P[a:b]
        eq = np.flatnonzero(np.any(rows != rows[0], axis=0))
        if len(eq):
            out.append((s, eq))
    return out


def hf_exact(P, mrow, p, x, sets=None):
    """(H, B) at the trimmed weights x, np.longdouble, dense symmetric"""
    n = P.shape[1]
    # the two non-negative sums apart (their rounding is 2^-64-relative to B,
    # seven orders below TOL): E2 = sum p E[c_j c_k], MM = sum p E[c_j] E[c_k]
    E2 = np.zeros((n, n), dtype=LD)
    MM = np.zeros((n, n), dtype=LD)
    lw = P.astype(LD) @ np.asarray(x, dtype=LD)
    p = np.asarray(p, dtype=LD)
    for s, eq in (equivocal_sets(P, mrow) if sets is None else sets):
        a, b = int(mrow[s]), int(mrow[s + 1])
        c = P[a:b][:, eq].astype(LD)
        e = np.exp(lw[a:b] - lw[a:b].max())
        r = e / e.sum()
        m = r @ c
        ix = np.ix_(eq, eq)
        MM[ix] += np.outer(p[s] * m, m)
        # sum_l p r_l c_l c_l^T: for a string of few paths path by path, over
        # each path's own non-zero columns (the same sum, far fewer terms)
        if b - a <= 8:
            for l in range(b - a):
                z = np.flatnonzero(c[l])
                E2[np.ix_(eq[z], eq[z])] += np.outer(p[s] * r[l] * c[l, z], c[l, z])
        else:
            E2[ix] += (c * (p[s] * r)[:, None]).T @ c
    return E2 - MM, E2 + MM


def dense(n, pairs, values):
    """the device's (pairs, values) scattered into a dense symmetric matrix
    and the mask of the entries it reported"""
    D = np.zeros((n, n))
    seen = np.zeros((n, n), dtype=bool)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    assert len(pairs) == len(values)
    lo, hi = pairs.min(axis=1), pairs.max(axis=1)
    assert len(np.unique(lo * n + hi)) == len(pairs), "a pair reported twice (as (j, k) and again, or as (k, j))"
    D[pairs[:, 0], pairs[:, 1]] = values
    D[pairs[:, 1], pairs[:, 0]] = values
    seen[pairs[:, 0], pairs[:, 1]] = True
    seen[pairs[:, 1], pairs[:, 0]] = True
    return D, seen


def worst_ratio(D, H, B):
    """max |D - H| / B over B > 0; asserts D == 0 wherever B == 0"""
    on = B > 0
    assert not np.any(D[~on] != 0.0), "a value outside the pattern of equivocal pairs"
    return float((np.abs(D.astype(LD) - H)[on] / B[on]).max()) if on.any() else 0.0


# -- the cases -----------------------------------------------------------------

N16 = dict(n_states=16, degree=3, vocab=4, emissions=2, n_strings=100, max_len=12, seed=3)


def ladder_text(K, m_max):
    """`^` branches to K disjoint chains c{k}_{i}, i < m_max; every chain state
    emits a or b and goes on along its chain or to `$`: a string over {a, b}
    of length m <= m_max has exactly K paths, no two sharing a parameter"""
    t = ["", "^", "$", "^  0", "^ " + " ".join(f"c{k}_0 0" for k in range(K))]
    for k in range(K):
        for i in range(m_max):
            t.append(f"c{k}_{i} a 0 b 0")
            t.append(f"c{k}_{i} " + (f"c{k}_{i + 1} 0 " if i + 1 < m_max else "") + "$ 0")
    return "\n".join(t) + "\n"


def _pack(strings):
    sym = np.frombuffer(b"".join(strings), dtype=np.uint8).copy()
    off = np.concatenate([[0], np.cumsum([len(s) for s in strings])]).astype(np.int64)
    return sym, off, np.ones(len(strings))


def ladder_corpus(m_max, seed=5):
    """two random strings of every length 1 .. m_max, then a^m_max and b^m_max
    (so every emission and every transition of every chain is used)"""
    rng = np.random.default_rng(seed)
    strings = []
    for m in range(1, m_max + 1):
        for _ in range(2):
            strings.append(bytes(rng.choice([97, 98], size=m).astype(np.uint8)))
    strings += [b"a" * m_max, b"b" * m_max]
    return strings


def ladder_corpus_many(m_max, n, lo, seed=7):
    """n random strings of lengths lo .. m_max, every length present"""
    rng = np.random.default_rng(seed)
    lens = np.concatenate([np.arange(lo, m_max + 1), rng.integers(lo, m_max + 1, size=n)])[:n]
    strings = [bytes(rng.choice([97, 98], size=int(m)).astype(np.uint8)) for m in lens]
    return strings


@functools.lru_cache(maxsize=None)
def ladder(K, m_max, many=0):
    from decode_cases import _reference
    strings = ladder_corpus(m_max)
    if many:
        strings = ladder_corpus_many(m_max, many, 8) + strings
    sym, off, wt = _pack(strings)
    return _reference(ladder_text(K, m_max), sym, off, wt)


@functools.lru_cache(maxsize=None)
def synthetic(name):
    import wfsa_amd as W
    from decode_cases import _family, _reference
    if name == "amb12":
        return _family("amb12")
    syn = W.Synthetic(**N16)
    sym, off, wt = syn.corpus()
    return _reference(syn.wfsa_text, sym, off, wt)


# name -> (constructor, largest |V_s| the case must show)
CASES = {
    "amb12": (lambda: synthetic("amb12"), 72),
    "n16": (lambda: synthetic("n16"), 86),
    "ladder4x16": (lambda: ladder(4, 16), 128),
    "ladder4x17": (lambda: ladder(4, 17), 136),
    "ladder4x32": (lambda: ladder(4, 32), 256),
    "ladder4x64": (lambda: ladder(4, 64), 512),
    "ladder3x10": (lambda: ladder(3, 10), 60),
    "ladder4x64_700": (lambda: ladder(4, 64, 700), 512),
}


def case(name):
    return CASES[name][0]()


@functools.lru_cache(maxsize=None)
def sets_of(name):
    ref = case(name)
    return equivocal_sets(ref["P"], ref["mrow"])


def draws(ref, seed=11, n=3):
    """the weight draws every test of a case uses (normal(-1, 0.5))"""
    rng = np.random.default_rng(seed)
    return [rng.normal(-1.0, 0.5, size=ref["o"].n) for _ in range(n)]
