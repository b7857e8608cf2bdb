"""What the sampling tests share (test_sample_reference.py,
test_gpu_sample_paths.py): a numpy restatement of the generator the sampler's
contract names (Philox4x32-10 and the 53-bit uniform, include/wfsa_dev.h), the
exact posterior of every string from the oracle's enumerated paths
(decode_cases: P, mrow) grouped by distinct count row -- two paths of a string
may share a row, and the device returns parameter ids, i.e. rows -- and the
goodness-of-fit statistic of the distribution test -- test infrastructure."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)

# the distribution test: cases, samples per call and seeds (64 x 16 = 1,024 draws per string)
DIST_CASES = ["amb12", "wide200", "long64"]
DIST_N = 64
DIST_SEEDS = list(range(101, 117))
DIST_WEIGHT_SEED = 23


def philox4x32_10(counter, key):
    """counter: four uint32 (arrays broadcast), key: two -> four uint32 arrays"""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF))
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0 = (k0 + np.uint64(W0)) & MASK
        k1 = (k1 + np.uint64(W1)) & MASK
    return [v.astype(np.uint32) for v in c]


def uniforms(seed, string, sample, n_draws):
    """u of draws 0 .. n_draws - 1: key (lo32(seed), hi32(seed)), counter
    (lo32(string), hi32(string), sample, d), u = (((x0 << 32) | x1) >> 11) 2^-53"""
    d = np.arange(n_draws, dtype=np.uint64)
    x = philox4x32_10((string & 0xFFFFFFFF, (string >> 32) & 0xFFFFFFFF, sample, d), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    bits = ((x[0].astype(np.uint64) << np.uint64(32)) | x[1].astype(np.uint64)) >> np.uint64(11)
    return bits.astype(np.float64) * 2.0 ** -53


def path_weights(P, x):
    """the oracle weight of every path: x . P over the columns with a positive
    count only (a plain P @ x turns 0 * -inf into NaN)"""
    with np.errstate(invalid="ignore"):
        return np.where(P > 0, P * x, 0.0).sum(axis=1)


def logsumexp(v):
    v = np.asarray(v, dtype=np.float64)
    m = v.max()
    if not np.isfinite(m):
        return m
    return m + np.log(np.exp(v - m).sum())


def posterior_cells(ref, x):
    """per recognized string r (mrow's order): (keys, prob, mult) -- keys maps
    a distinct count row's bytes (int64, P's columns) to its cell, prob[cell] =
    the exact posterior mass of the paths with that row at x, mult[cell] = how
    many paths have it"""
    P, mrow = ref["P"], ref["mrow"]
    lw = path_weights(P, x)
    cells = []
    for r in range(len(mrow) - 1):
        a, b = mrow[r], mrow[r + 1]
        w = lw[a:b]
        p = np.exp(w - logsumexp(w)) if np.isfinite(w).any() else np.zeros(b - a)
        keys, prob, mult = {}, [], []
        for l in range(a, b):
            key = P[l].astype(np.int64).tobytes()
            if key not in keys:
                keys[key] = len(prob)
                prob.append(0.0)
                mult.append(0)
            prob[keys[key]] += p[l - a]
            mult[keys[key]] += 1
        cells.append((keys, np.array(prob), np.array(mult, dtype=np.float64)))
    return cells


def chi_square(cells, counts, n):
    """X^2 = sum (O - E)^2 / E and dof = sum (cells - 1) over the strings,
    counts[r][cell] = the observed draws of n per string; cells with E < 5 are
    merged into one rest cell per string, strings left with one cell dropped.
    Also returns the draws that fell in a cell of posterior 0."""
    x2, dof, impossible = 0.0, 0, 0
    for (keys, prob, _), obs in zip(cells, counts):
        obs = np.asarray(obs, dtype=np.float64)
        assert obs.shape == prob.shape and obs.sum() == n
        impossible += int(obs[prob == 0.0].sum())
        e = n * prob
        big = e >= 5.0
        E, O = list(e[big]), list(obs[big])
        if (~big).any():
            E.append(e[~big].sum())
            O.append(obs[~big].sum())
        E, O = np.array(E), np.array(O)
        keep = E > 0
        E, O = E[keep], O[keep]
        if len(E) < 2:
            continue
        x2 += float(((O - E) ** 2 / E).sum())
        dof += len(E) - 1
    return x2, dof, impossible


def bound(dof):
    """a correct sampler's X^2 has mean dof and standard deviation sqrt(2 dof)"""
    return dof + 6.0 * np.sqrt(2.0 * dof)


def draw_counts(cells, n, rng, prob_of=None):
    """numpy draws: n per string from prob_of(r, prob, mult) (default: the
    exact posterior), as counts per cell"""
    out = []
    for r, (_, prob, mult) in enumerate(cells):
        p = prob if prob_of is None else prob_of(r, prob, mult)
        out.append(rng.multinomial(n, p / p.sum()))
    return out


def dist_weights(ref, perm=None):
    """the distribution test's one weight draw for a case: trimmed x, and the
    device's w_full for it when the device's parameter order is given"""
    o = ref["o"]
    x = np.random.default_rng(DIST_WEIGHT_SEED).normal(-1.0, 0.5, size=o.n)
    if perm is None:
        return x
    o.set_x(x)
    return x, o.w_full()[perm]
