"""What the byte-marginal tests share (test_marginal_reference.py,
test_gpu_byte_marginals.py): a plain enumeration of the accepting paths of a
string, straight from the flattened automaton (Fsa.desc()), by the rule
trellis_model.hpp describes -- follow a transition, then an emission of the
target that is a prefix of the rest of the word; take the end transition only
when the word is consumed -- with the parameter list and the state of every byte
of each path, and what follows from them per string at given weights: log q, the
per-byte state masses, the boundary probabilities and the score of every path
under the max-expected-accuracy criterion -- test infrastructure."""
import numpy as np

import sample_reference as R


def model(fsa):
    """the automaton as plain lists, in desc()'s numbering"""
    d = fsa.desc()
    n = d.n_states
    em_ptr = [d.em_ptr[i] for i in range(n + 1)]
    tr_ptr = [d.tr_ptr[i] for i in range(n + 1)]
    n_em, n_tr = em_ptr[n], tr_ptr[n]
    em = []
    for e in range(n_em):
        o, l = d.em_off[e], d.em_len[e]
        em.append((bytes(d.em_bytes[o + k] for k in range(l)), d.em_param[e]))
    tr = [(d.tr_dst[t], d.tr_param[t]) for t in range(n_tr)]
    return dict(n_states=n, start=d.start, end=d.end, n_params=d.n_params, em_ptr=em_ptr, tr_ptr=tr_ptr, em=em, tr=tr)


def paths(m, word):
    """every accepting path of `word` (bytes): (parameter ids in path order, -1s
    left out; the emitting state of every byte; whether an emission ends there)"""
    out = []
    L = len(word)
    em_ptr, tr_ptr, em, tr, end = m["em_ptr"], m["tr_ptr"], m["em"], m["tr"], m["end"]

    def walk(state, pos, params, states, ends):
        for t in range(tr_ptr[state], tr_ptr[state + 1]):
            target, tp = tr[t]
            if target == end:
                if pos == L:
                    out.append((params + [tp] if tp >= 0 else params, states, ends))
                continue
            for e in range(em_ptr[target], em_ptr[target + 1]):
                text, ep = em[e]
                if word[pos:pos + len(text)] != text:
                    continue
                k = len(text)
                walk(target, pos + k, params + [p for p in (tp, ep) if p >= 0], states + [target] * k,
                     ends + [False] * (k - 1) + [True] * min(k, 1))

    walk(m["start"], 0, [], [], [])
    return out


def enumerate_corpus(fsa, sym, off):
    """per string: n (paths), params (list of id lists), C (path x parameter
    counts), states and ends (path x byte)"""
    m = model(fsa)
    sym = np.asarray(sym, dtype=np.uint8).tobytes()
    res = []
    for s in range(len(off) - 1):
        word = sym[off[s]:off[s + 1]]
        ps = paths(m, word)
        C = np.zeros((len(ps), max(m["n_params"], 1)), dtype=np.int32)
        for l, (params, _, _) in enumerate(ps):
            np.add.at(C[l], params, 1)
        res.append(dict(n=len(ps), L=len(word), params=[p[0] for p in ps], C=C,
                        states=np.array([p[1] for p in ps], dtype=np.int64).reshape(len(ps), len(word)),
                        ends=np.array([p[2] for p in ps], dtype=bool).reshape(len(ps), len(word))))
    return dict(n_states=m["n_states"], strings=res)


def weights(entry, w_full):
    """the log weight of every path: the sum of w_full over its parameters (-1 parameters weigh 0)"""
    w = np.zeros(entry["C"].shape[1])
    w[:len(w_full)] = np.asarray(w_full, dtype=np.float64)[:len(w)]
    return R.path_weights(entry["C"], w)


def derive(entry, w_full, n_states):
    """logq; prob (path posteriors, 0 for a path of weight -inf); mass [L, n_states];
    boundary [L]; score (per path: the sum over its bytes of the mass of its state
    there; NaN for a path of weight -inf); best (the greatest score); lw.
    A string without a path of finite weight: logq -inf, the rest None."""
    lw = weights(entry, w_full)
    keep = np.isfinite(lw)
    if not keep.any():
        return dict(logq=-np.inf, lw=lw, prob=None, mass=None, boundary=None, score=None, best=None)
    lq = R.logsumexp(lw[keep])
    prob = np.where(keep, np.exp(np.where(keep, lw, 0.0) - lq), 0.0)
    L = entry["L"]
    mass = np.zeros((L, n_states))
    for i in range(L):
        np.add.at(mass[i], entry["states"][:, i], prob)
    boundary = (prob[:, None] * entry["ends"]).sum(axis=0)
    score = np.array([mass[np.arange(L), entry["states"][l]].sum() if keep[l] else np.nan for l in range(entry["n"])])
    return dict(logq=lq, lw=lw, prob=prob, mass=mass, boundary=boundary, score=score, best=np.nanmax(score))
