"""Numpy restatement of the dense path's posterior path sampler
(wfsa_dev_dense_sample_paths, include/wfsa_dev.h), per string in float64:
the forward pass scaled at every step (alpha_1 = a (.) E, alpha_{j+1} =
(alpha_j A / sum alpha_j) (.) E), the uniforms of sample_reference.uniforms,
every choice in ascending state order over the np padded candidates by plain
left-to-right running sums (np.cumsum), the ids and logw as
dense_decode_reference.decode forms them.

The device sums its candidates in groups of 64 (a butterfly per group, then
left to right), so its running sums differ from these by rounding -- about
np eps relative.  For every sample the restatement therefore also returns its
margin: the smallest, over the sample's choices, of |u total - nearest
running-sum boundary| / total.  A sample whose margin is at least MARGIN must
be the same path on the device; the others are exempt, and
test_dense_sample_reference.py checks on the CPU that they are under 1% of
every case the GPU tests compare path for path -- test infrastructure."""
import numpy as np

import sample_reference as SR
from dense_decode_reference import Tables

TILE = 128      # kDenseTile: the states are padded to a multiple of it
MARGIN = 1e-9   # the decision width below which a sample is exempt
EXEMPT = 0.01   # the share of samples that may be exempt


class ExpTables:
    """exp of dense_decode_reference.Tables' log tables, padded to np states:
    exp(w) for a parameter, 1 for a single-member group, 0 for no edge or a
    padded state"""

    def __init__(self, fsa, w):
        self.tab = t = Tables(fsa, w)
        self.n = t.n
        self.np = npad = -(-t.n // TILE) * TILE
        with np.errstate(under="ignore"):
            self.A = np.zeros((npad, npad))
            self.A[:t.n, :t.n] = np.exp(t.lA)
            self.E = np.zeros((npad, 256))
            self.E[:t.n] = np.exp(t.lE)
            self.a0, self.aend = np.zeros(npad), np.zeros(npad)
            self.a0[:t.n] = np.exp(t.l0)
            self.aend[:t.n] = np.exp(t.lend)
            self.se = float(np.exp(t.lse))


def choose(a, b, u):
    """(state, margin) of one choice among the masses a[S] b[S] in ascending
    S: the first whose running sum exceeds u total; when rounding leaves
    none, the last of positive mass; when the total is 0, the lowest S with
    both factors positive; -1: no candidate"""
    m = a * b
    cs = np.cumsum(m)
    total = cs[-1]
    if not total > 0.0:
        both = np.flatnonzero((a > 0.0) & (b > 0.0))
        return (int(both[0]) if len(both) else -1), np.inf
    x = u * total
    over = np.flatnonzero(cs > x)
    k = int(over[0]) if len(over) else int(np.flatnonzero(m > 0.0)[-1])
    return k, float(np.abs(cs - x).min() / total)


def forward(et, s):
    """(alpha [L][np] scaled rows, log q) of one non-empty string"""
    L = len(s)
    al = np.zeros((L, et.np))
    la = 0.0
    with np.errstate(divide="ignore", under="ignore"):
        al[0] = et.a0 * et.E[:, s[0]]
        for j in range(1, L):
            z = al[j - 1].sum()
            la += np.log(z)
            al[j] = (al[j - 1].dot(et.A) * (1.0 / z if z > 0.0 else 0.0)) * et.E[:, s[j]]
        fin = al[L - 1].dot(et.aend)
        logq = la + np.log(fin)
    return al, (float(logq) if logq > -np.inf else -np.inf)


def sample_string(et, s, index, n, seed):
    """one string (bytes as integers) at corpus index `index`: (log q, [(logw,
    ids, margin)] per sample -- n of them, or none when the string has no path)"""
    tab = et.tab
    L = len(s)
    if L == 0:
        if tab.pse == -2:
            return -np.inf, []
        total = 0.0 + tab.edge_lw(tab.pse)
        with np.errstate(divide="ignore"):
            logq = float(np.log(et.se))
        if not (total > -np.inf and logq > -np.inf):
            return -np.inf, []
        ids = np.array([tab.pse] if tab.pse >= 0 else [], dtype=np.int32)
        return logq, [(total, ids, np.inf)] * n
    al, logq = forward(et, s)
    if not logq > -np.inf:
        return -np.inf, []
    out = []
    for t in range(n):
        u = SR.uniforms(seed, index, t, L)
        cur, margin = choose(al[L - 1], et.aend, u[0])
        assert cur >= 0
        states = [cur]
        for j in range(L - 1, 0, -1):   # draw L - j: the state at byte j - 1 (from 0)
            cur, mg = choose(al[j - 1], et.A[:, cur], u[L - j])
            assert cur >= 0
            margin = min(margin, mg)
            states.append(cur)
        states.reverse()
        ids, total, prev = [], 0.0, -1
        for j, T in enumerate(states):
            assert T < tab.n
            pt = tab.p0[T] if j == 0 else tab.pA[prev, T]
            pe = tab.pE[T, s[j]]
            assert pt != -2 and pe != -2
            total += tab.edge_lw(pt, pe)
            ids += [p for p in (pt, pe) if p >= 0]
            prev = T
        assert tab.pend[prev] != -2
        total += tab.edge_lw(tab.pend[prev])
        if tab.pend[prev] >= 0:
            ids.append(tab.pend[prev])
        out.append((total, np.array(ids, dtype=np.int32), margin))
    return logq, out


def sample_corpus(fsa, w, sym, off, n, seed):
    """every string: (srow [S + 1], logw, prow, pidx, logq [S], margin per
    path) in sample_paths' layout"""
    et = ExpTables(fsa, w)
    S = len(off) - 1
    srow, logq = np.zeros(S + 1, dtype=np.int64), np.empty(S)
    logw, margin, parts = [], [], []
    for i in range(S):
        logq[i], samples = sample_string(et, np.asarray(sym[off[i]:off[i + 1]], dtype=np.int64), i, n, seed)
        for lw, ids, mg in samples:
            logw.append(lw)
            margin.append(mg)
            parts.append(ids)
        srow[i + 1] = len(logw)
    prow = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    pidx = np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, dtype=np.int32)
    return srow, np.array(logw), prow, pidx, logq, np.array(margin)


# -- the cases the GPU tests compare path for path ------------------------------------

N_PATHS = 5       # samples per string against the restatement
N_TRELLIS = 8     # against the trellis sampler
SEED = 20240229
TILE_SPECS = {
    # 200 states: np = 256, four groups of 64, two column tiles, padded states
    "tiles200": (dict(n_states=200, vocab=5, emissions=2, n_strings=300, max_len=40, seed=12), 8),
    # 64 states x 600 strings: several strings per slot, two row tiles
    "slots64": (dict(n_states=64, vocab=8, emissions=3, n_strings=600, max_len=12, seed=13), 9),
}
GADGET_CASES = ("holes12", "seams", "edge129", "peaked", "long300")


def case(name):
    """(fsa, w, sym, off, p) of a named case: a dense_decode_reference
    BYTE_CASES model with its weight draw, one of TILE_SPECS, or a gadget of
    dense_gadgets with its own weights"""
    import wfsa_amd as W
    import dense_decode_reference as R
    if name in R.BYTE_CASES:
        text, sym, off, wt = R.synthetic(name)
        fsa = W.Fsa.read_text(text)
        return fsa, R.case_weights(name, len(fsa.param_names())), sym, off, wt / wt.sum()
    if name in TILE_SPECS:
        spec, seed = TILE_SPECS[name]
        syn = W.Synthetic(degree=1, dense=True, **spec)
        sym, off, wt = syn.corpus()
        fsa = W.Fsa.read_text(syn.wfsa_text)
        return fsa, np.random.default_rng(seed).normal(-1.0, 0.5, size=len(fsa.param_names())), sym, off, wt / wt.sum()
    import dense_gadgets as G
    g = G.GADGETS[name]()
    fsa = W.Fsa.read_text(g.text.encode("latin-1"))
    return fsa, G.weights(g, fsa.param_names()), g.sym, g.off, g.p


def without_a_path_case():
    """test_dense_best_paths_without_a_path's weights and corpus: dense16 with
    the most-used quarter of the parameters at -inf, an empty string and a
    string with a byte no state emits appended"""
    import wfsa_amd as W
    import dense_decode_reference as R
    text, sym, off, wt = R.synthetic("dense16")
    fsa = W.Fsa.read_text(text)
    n_par = len(fsa.param_names())
    w = R.case_weights("dense16", n_par)
    _, _, pidx0, _, _ = R.decode_corpus(fsa, w, sym, off)
    used = np.bincount(pidx0, minlength=n_par)
    w[np.argsort(-used, kind="stable")[:n_par // 4]] = -np.inf
    strings = [bytes(sym[off[i]:off[i + 1]]) for i in range(len(wt))]
    strings += [b"", strings[0][:1] + b"\xff" + strings[0][1:]]
    sym2 = np.frombuffer(b"".join(strings), dtype=np.uint8).copy()
    off2 = np.concatenate([[0], np.cumsum([len(s) for s in strings])]).astype(np.int64)
    wt2 = np.concatenate([wt, [1.0, 1.0]])
    return fsa, w, sym2, off2, wt2 / wt2.sum()


# (case, n) of every comparison of paths with the restatement or the trellis sampler
PATH_CASES = [(nm, N_PATHS) for nm in ("dense16", "auto128", "tiles200", "slots64") + GADGET_CASES] + \
             [(nm, N_TRELLIS) for nm in ("dense16", "auto128")]

_MEMO = {}


def expected(name, n, seed=SEED):
    """sample_corpus of a case, computed once and left unchanged"""
    key = (name, n, seed)
    if key not in _MEMO:
        fsa, w, sym, off, p = case(name)
        res = sample_corpus(fsa, w, sym, off, n, seed)
        for a in res:
            a.setflags(write=False)
        _MEMO[key] = res
    return _MEMO[key]
