"""What the generation tests share (test_generate_reference.py,
test_gpu_generate.py): a numpy walker of the contract of wfsa_dev_generate
(include/wfsa_dev.h) over Fsa.desc(), with sample_reference's generator -- all
samples step together, a choice is the contract's rule (first running sum above
u * T, else the last candidate of positive mass) found by bisection over the
left-to-right running sums -- plus the hand-written automata, the
group-normalised weights and the goodness-of-fit statistic of the distribution
test -- test infrastructure."""
import numpy as np

import sample_reference as R

SAMPLE_WORD = 0xFFFFFFFF
NEAR = 1e-9

# the distribution test: amb12 at group-normalised weights
DIST_CASE = "amb12"
DIST_N = 65536
DIST_MAX_LEN = 8
DIST_SEEDS = [201, 202]
DIST_WEIGHT_SEED = 31


def model_arrays(fsa):
    """copies of Fsa.desc()'s arrays"""
    d = fsa.desc()
    n = d.n_states

    def arr(p, count, dtype):
        return np.ctypeslib.as_array(p, shape=(max(count, 1),))[:count].astype(dtype, copy=True)

    em_ptr = arr(d.em_ptr, n + 1, np.int64)
    tr_ptr = arr(d.tr_ptr, n + 1, np.int64)
    n_em, n_tr = int(em_ptr[-1]), int(tr_ptr[-1])
    em_off = arr(d.em_off, n_em, np.int64)
    em_len = arr(d.em_len, n_em, np.int64)
    n_bytes = int((em_off + em_len).max()) if n_em else 0
    return dict(n_states=n, start=d.start, end=d.end, n_params=d.n_params, em_ptr=em_ptr, em_off=em_off, em_len=em_len,
                em_param=arr(d.em_param, n_em, np.int64), em_bytes=arr(d.em_bytes, n_bytes, np.uint8), tr_ptr=tr_ptr,
                tr_dst=arr(d.tr_dst, n_tr, np.int64), tr_param=arr(d.tr_param, n_tr, np.int64))


def _mass(param, w):
    a = np.ones(len(param))
    has = param >= 0
    with np.errstate(over="ignore"):
        a[has] = np.exp(w[param[has]])
    return a


def running_sums(ptr, param, w):
    """inclusive left-to-right sums of the masses within every state's group"""
    a = _mass(param, w)
    cdf = np.zeros(len(a))
    for u in range(len(ptr) - 1):
        s = 0.0
        for k in range(ptr[u], ptr[u + 1]):
            s += a[k]
            cdf[k] = s
    return cdf


def _choose(cdf, param, w, lo, hi, T, u):
    """the contract's choice for every row: (k, near-tie flag)"""
    with np.errstate(invalid="ignore", over="ignore"):
        x = u * T
    l, h = lo.copy(), hi.copy()
    while True:
        act = np.flatnonzero(l < h)
        if not len(act):
            break
        mid = l[act] + ((h[act] - l[act]) >> 1)
        above = cdf[mid] > x[act]
        h[act] = np.where(above, mid, h[act])
        l[act] = np.where(above, l[act], mid + 1)
    for r in np.flatnonzero(l == hi):   # (u * T rounded up to T): the last candidate of positive mass
        k = hi[r] - 1
        while k > lo[r] and not _mass(param[k:k + 1], w)[0] > 0.0:
            k -= 1
        l[r] = k
    # the running sums next to u * T: the first above it and the last not above it
    k_hi = np.minimum(l, hi - 1)
    k_lo = np.maximum(np.minimum(l, hi) - 1, lo)
    with np.errstate(invalid="ignore"):
        near = (np.abs(cdf[k_hi] - x) <= NEAR * T) | (np.abs(cdf[k_lo] - x) <= NEAR * T)
    return l, near


class _Draws:
    """u of draw d of sample i, d < n_draws for all samples at once; more draws
    (a walk with empty emissions) are made when asked for"""

    def __init__(self, seed, n, n_draws):
        self.seed, self.n = seed, n
        self.table = R.uniforms(seed, np.arange(n, dtype=np.int64)[:, None], SAMPLE_WORD, n_draws)

    def __call__(self, ids, d):
        while d >= self.table.shape[1]:
            self.table = R.uniforms(self.seed, np.arange(self.n, dtype=np.int64)[:, None], SAMPLE_WORD, 2 * self.table.shape[1])
        return self.table[ids, d]


def generate(fsa, w_full, n, max_len, seed):
    """the device's outputs (sym, off, logw, logp, status, prow, pidx) plus, per
    sample, `near` (some choice had a running sum within 1e-9 T of u T: one ulp
    in exp may pick another candidate) and `steps` (choices made)"""
    M = fsa if isinstance(fsa, dict) else model_arrays(fsa)
    w = np.asarray(w_full, dtype=np.float64)
    assert not (np.isnan(w) | (w == np.inf)).any()
    cdf = {"tr": running_sums(M["tr_ptr"], M["tr_param"], w), "em": running_sums(M["em_ptr"], M["em_param"], w)}
    max_steps = M["n_states"] * (max_len + 1)
    assert 2 * max_steps < 2 ** 32
    U = np.full(n, M["start"], dtype=np.int64)
    length = np.zeros(n, dtype=np.int64)
    logw, logp = np.zeros(n), np.zeros(n)
    status = np.full(n, -1, dtype=np.int64)
    near = np.zeros(n, dtype=bool)
    steps = np.zeros(n, dtype=np.int64)
    draws = _Draws(seed, n, 2 * (max_len + 2))
    events = []   # recorded choices: (samples, draw index, parameter, emission or -1)

    def choose(kind, ids, state, draw):
        """one choice of `kind` for the samples ids at `state`: the samples
        that had one (the others are dead), their candidate and its group's T"""
        ptr, param = M[kind + "_ptr"], M[kind + "_param"]
        lo, hi = ptr[state], ptr[state + 1]
        T = np.zeros(len(ids))
        some = hi > lo
        T[some] = cdf[kind][hi[some] - 1]
        ok = T > 0.0
        status[ids[~ok]] = 2
        ids, lo, hi, T = ids[ok], lo[ok], hi[ok], T[ok]
        k, nr = _choose(cdf[kind], param, w, lo, hi, T, draws(ids, draw))
        near[ids] |= nr
        steps[ids] += 1
        return ok, ids, k, T

    def record(ids, draw, p, T, em):
        wk = np.zeros(len(ids))
        has = p >= 0
        wk[has] = w[p[has]]
        logw[ids[has]] += wk[has]
        logp[ids] += wk - np.log(T)
        events.append((ids, np.full(len(ids), draw, dtype=np.int64), p, em))

    m = 0
    while True:
        ids = np.flatnonzero(status < 0)
        if not len(ids):
            break
        if m >= max_steps:   # (never, without an epsilon cycle)
            status[ids] = 1
            break
        _, ids, k, T = choose("tr", ids, U[ids], 2 * m)
        record(ids, 2 * m, M["tr_param"][k], T, np.full(len(ids), -1, dtype=np.int64))
        V = M["tr_dst"][k]
        done = V == M["end"]
        status[ids[done]] = 0
        ids, V = ids[~done], V[~done]
        ok, ids, k, T = choose("em", ids, V, 2 * m + 1)
        V = V[ok]
        L = M["em_len"][k]
        cut = L > max_len - length[ids]
        status[ids[cut]] = 1   # truncated: that emission is not recorded
        ids, V, k, T, L = ids[~cut], V[~cut], k[~cut], T[~cut], L[~cut]
        record(ids, 2 * m + 1, M["em_param"][k], T, k)
        length[ids] += L
        U[ids] = V
        m += 1
    # the recorded choices in (sample, draw) order
    if events:
        es, ed, ep, ee = (np.concatenate([e[j] for e in events]) for j in range(4))
    else:
        es = ed = ep = ee = np.zeros(0, dtype=np.int64)
    order = np.lexsort((ed, es))
    es, ep, ee = es[order], ep[order], ee[order]
    has = ep >= 0
    prow = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(es[has], minlength=n), out=prow[1:])
    pidx = ep[has].astype(np.int32)
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(length, out=off[1:])
    ems = ee[ee >= 0]
    el = M["em_len"][ems]
    first = np.cumsum(el) - el   # where each recorded emission's bytes begin in sym
    sym = M["em_bytes"][np.repeat(M["em_off"][ems] - first, el) + np.arange(int(el.sum()))].astype(np.uint8)
    assert len(sym) == off[-1]
    return dict(sym=sym, off=off, logw=logw, logp=logp, status=status.astype(np.int8), prow=prow, pidx=pidx, near=near, steps=steps)


def strings(out):
    sym, off = out["sym"].tobytes(), out["off"]
    return [sym[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def normalised(fsa, w_full):
    """w_full with log T of its group taken from every member: each state's
    transitions and each state's emissions then sum to 1 (a parameter belongs
    to one group)"""
    M = fsa if isinstance(fsa, dict) else model_arrays(fsa)
    w = np.array(w_full, dtype=np.float64)
    out = w.copy()
    for kind in ("tr", "em"):
        ptr, param = M[kind + "_ptr"], M[kind + "_param"]
        for u in range(M["n_states"]):
            p = param[ptr[u]:ptr[u + 1]]
            if len(p) and (p >= 0).all():
                out[p] = w[p] - R.logsumexp(w[p])
    return out


def chi_square(counts, expect, rest_observed, n):
    """X^2 and dof of observed counts against expectations (one cell per
    distinct string); cells with expectation below 5 and `rest_observed` (the
    truncated and dead samples, strings outside the cells) form one rest cell
    whose expectation is what is left of n"""
    counts, expect = np.asarray(counts, dtype=np.float64), np.asarray(expect, dtype=np.float64)
    big = expect >= 5.0
    E, O = list(expect[big]), list(counts[big])
    rest_e = n - expect[big].sum()
    rest_o = counts[~big].sum() + rest_observed
    assert abs(sum(O) + rest_o - n) < 0.5
    if rest_e > 0:
        E.append(rest_e)
        O.append(rest_o)
    else:
        assert rest_o == 0
    E, O = np.array(E), np.array(O)
    return float(((O - E) ** 2 / E).sum()), len(E) - 1


def wfsa_text(states, start="^", end="$"):
    """a .wfsa text (separator " ") from {state: ([(emission, weight)],
    [(target, weight)])}; the start state emits the empty string"""
    lines = ["", start, end]
    for name, (em, tr) in states.items():
        lines.append(" ".join([name] + [t for e, w in em for t in (e, repr(float(w)))]))
        lines.append(" ".join([name] + [t for d, w in tr for t in (d, repr(float(w)))]))
    return "\n".join(lines) + "\n"


def fan(k):
    """start -> one of k states with equal weights, state i emitting the two
    bytes of "%02x" % i and going to the end: a transition group of k (k = 1: a
    single-member group, param -1); every other group has one member"""
    states = {"^": ([("", 0.0)], [("s%d" % i, -1.0) for i in range(k)])}
    for i in range(k):
        states["s%d" % i] = ([("%02x" % i, 0.0)], [("$", 0.0)])
    return wfsa_text(states)


# empty, 1-, 2- and 3-byte emissions: A emits "" or "a", B "bc" or "def", both loop or stop
EMISSIONS = wfsa_text({
    "^": ([("", 0.0)], [("A", -0.5), ("B", -1.0)]),
    "A": ([("", -1.0), ("a", -0.7)], [("B", -0.9), ("$", -0.6)]),
    "B": ([("bc", -0.8), ("def", -0.6)], [("A", -1.2), ("$", -0.4)]),
})

# no loop: ^ -> A | B, A -> B | $, B -> $ ; B's two emissions die when both are at -inf
TINY = wfsa_text({
    "^": ([("", 0.0)], [("A", -0.3), ("B", -1.4)]),
    "A": ([("x", -0.2), ("yy", -1.9)], [("B", -0.7), ("$", -0.8)]),
    "B": ([("p", -1.1), ("q", -0.5)], [("$", 0.0)]),
})


def params_of(fsa, state, kind):
    """the Fsa parameter ids of `state`'s emissions ("E") or transitions ("T"), in the model's order"""
    M = model_arrays(fsa)
    u = fsa.state_names().index(state)
    key = "em" if kind == "E" else "tr"
    return M[key + "_param"][M[key + "_ptr"][u]:M[key + "_ptr"][u + 1]]


def transition_param(fsa, src, dst):
    """the Fsa parameter id of the transition src -> dst (state names)"""
    M = model_arrays(fsa)
    names = fsa.state_names()
    u = names.index(src)
    for k in range(M["tr_ptr"][u], M["tr_ptr"][u + 1]):
        if names[M["tr_dst"][k]] == dst:
            return int(M["tr_param"][k])
    raise KeyError((src, dst))


def emission_param(fsa, state, text):
    """the Fsa parameter id of `state`'s emission `text` (bytes)"""
    M = model_arrays(fsa)
    u = fsa.state_names().index(state)
    for k in range(M["em_ptr"][u], M["em_ptr"][u + 1]):
        if M["em_bytes"][M["em_off"][k]:M["em_off"][k] + M["em_len"][k]].tobytes() == text:
            return int(M["em_param"][k])
    raise KeyError((state, text))


def dist_model():
    """the distribution test's automaton (text) and its group-normalised weights"""
    import wfsa_amd as W
    from decode_cases import _family
    text = _family(DIST_CASE)["text"]
    fsa = W.Fsa.read_text(text)
    w = np.random.default_rng(DIST_WEIGHT_SEED).normal(-1.0, 0.5, size=fsa.counts()["parameters"])
    return text, normalised(fsa, w)
