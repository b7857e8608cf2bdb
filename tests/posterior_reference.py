"""What the posterior-count tests share (test_posterior_reference.py,
test_gpu_posterior_counts.py): the exact per-string E-step from the oracle's
enumerated paths (decode_cases: P, mrow) -- log q, the expected count row
softmax(path weights of s) @ P[rows of s] and the entropy -sum p log p of every
recognized string at a trimmed x -- and the map from a device row (Fsa
parameter ids) to the oracle's columns -- test infrastructure."""
import numpy as np

import sample_reference as R


def posterior(ref, x):
    """per recognized string r (mrow's order): logq[r], counts[r] (dense, P's
    columns) and entropy[r]; a string without a path of finite weight has
    logq = -inf, a zero row and entropy NaN.  Paths of weight -inf carry no mass."""
    P, mrow = ref["P"], ref["mrow"]
    lw = R.path_weights(P, x)
    n = len(mrow) - 1
    logq = np.full(n, -np.inf)
    counts = np.zeros((n, P.shape[1]))
    entropy = np.full(n, np.nan)
    for r in range(n):
        a, b = mrow[r], mrow[r + 1]
        w = lw[a:b]
        keep = np.isfinite(w)
        if not keep.any():
            continue
        lq = R.logsumexp(w[keep])
        lp = w[keep] - lq
        p = np.exp(lp)
        logq[r] = lq
        counts[r] = p @ P[a:b][keep].astype(np.float64)
        entropy[r] = -(p * lp).sum()
    return logq, counts, entropy


def path_count(ref, x):
    """finite-weight paths of every recognized string at x"""
    mrow = ref["mrow"]
    lw = R.path_weights(ref["P"], x)
    return np.array([np.isfinite(lw[mrow[r]:mrow[r + 1]]).sum() for r in range(len(mrow) - 1)])


def device_rows(ref, perm, crow, cidx, cval, strings):
    """the device's sparse rows of `strings` as dense rows over the oracle's
    columns, and the mask of the columns each row lists.  No listed id may be a
    parameter the oracle trimmed away as unused (-2); ids the oracle holds
    fixed (-1) have no column and are left out."""
    tr = ref["trim"][perm[cidx]]
    assert (tr != -2).all()   # no unused parameter carries a count
    n_col = ref["P"].shape[1]
    dense = np.zeros((len(strings), n_col))
    listed = np.zeros((len(strings), n_col), dtype=bool)
    for r, s in enumerate(strings):
        a, b = crow[s], crow[s + 1]
        t = tr[a:b]
        np.add.at(dense[r], t[t >= 0], cval[a:b][t >= 0])
        listed[r, t[t >= 0]] = True
    return dense, listed


def cap(logq, lengths):
    """the parity cap of a string: a mass is exp of a three-term difference of
    log alphas, each within 1e-11 max(1, |log q|), chained over L + 1 steps"""
    return 3e-11 * np.maximum(1.0, np.abs(logq)) * (np.asarray(lengths) + 1.0)
