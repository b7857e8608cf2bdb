"""CPU tests of the reference the posterior-count tests rest on
(posterior_reference.py), on the golden models and amb12: the entropy identity
H_s = log q_s - E_s[count] . x, single-path strings, and the count rows against
the central finite difference of the oracle's trellis evaluation
(Oracle.trellis_eval, which enumerates nothing) in every x_j."""
import numpy as np
import pytest

import posterior_reference as PR
from decode_cases import GOLDEN, _source

CASES = [c[0] for c in GOLDEN] + ["amb12"]


def _x(ref):
    return np.random.default_rng(5).normal(-1.0, 0.5, size=ref["o"].n)


@pytest.mark.parametrize("name", CASES)
def test_entropy_identity_and_single_paths(name):
    ref = _source(name)
    x = _x(ref)
    logq, counts, entropy = PR.posterior(ref, x)
    assert np.isfinite(logq).all() and (entropy >= 0.0).all() and (counts >= 0.0).all()
    err = np.abs(entropy - (logq - counts @ x))
    print(name, "worst |H - (log q - E[count] . x)|:", err.max())
    assert (err <= 1e-12).all()
    P, mrow = ref["P"], ref["mrow"]
    single = np.flatnonzero(np.diff(mrow) == 1)
    if name in ("talk", "test3"):
        assert len(single) > 0
    for r in single:
        assert (counts[r] == P[mrow[r]]).all() and entropy[r] == 0.0


@pytest.mark.parametrize("name", CASES)
def test_rows_are_the_gradient_of_log_q(name):
    """d log q_s / d x_j = E_s[count_j], by central differences (h = 1e-5) of the
    trellis evaluation's log q.  Bound 1e-8: the truncation error is
    h^2 / 6 times a third cumulant of a count (1.7e-11 per unit of it) and the
    rounding error about eps |log q| / h = 1e-16 x 10 / 1e-5 = 1e-10; measured
    at most 4e-11 on the goldens and 1.1e-10 on amb12."""
    ref = _source(name)
    o = ref["o"]
    x = _x(ref)
    _, counts, _ = PR.posterior(ref, x)
    rec = ref["rec"]
    h = 1e-5
    worst = 0.0
    try:
        for j in range(o.n):
            lq = []
            for sgn in (1.0, -1.0):
                xx = x.copy()
                xx[j] += sgn * h
                o.set_x(xx)
                lq.append(o.trellis_eval(o.w_full())[1][rec])
            fd = (lq[0] - lq[1]) / (2.0 * h)
            worst = max(worst, np.abs(fd - counts[:, j]).max())
    finally:
        o.set_x(x)
    print(name, "worst |finite difference - count|:", worst)
    assert worst <= 1e-8
