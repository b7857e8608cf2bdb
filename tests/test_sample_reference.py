"""CPU tests of what the sampling tests rest on (sample_reference.py): the numpy
Philox4x32-10 against known answers, and the goodness-of-fit condition of the
distribution test (test_gpu_sample_paths.py) on the very cases, weights and
sample counts that test uses -- numpy draws from the exact posterior pass it,
draws uniform over each string's paths and draws from the posterior at other
weights fail it, and every case has at least 200 degrees of freedom."""
import numpy as np
import pytest

import sample_reference as R
from decode_cases import _family

KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_philox_known_answers(counter, key, want):
    got = R.philox4x32_10(counter, key)
    assert tuple(int(v) for v in got) == want


def test_uniform_mapping():
    """u is the top 53 bits of words 0 and 1, in [0, 1), one counter per draw"""
    u = R.uniforms(seed=(7 << 32) | 5, string=(3 << 32) | 9, sample=2, n_draws=4)
    for d in range(4):
        x = R.philox4x32_10((9, 3, 2, d), (5, 7))
        bits = ((int(x[0]) << 32) | int(x[1])) >> 11
        assert u[d] == bits * 2.0 ** -53 and 0.0 <= u[d] < 1.0
    # all-ones words give the largest value below 1
    assert ((0xFFFFFFFFFFFFFFFF >> 11) * 2.0 ** -53) == 1.0 - 2.0 ** -53


@pytest.mark.parametrize("name", R.DIST_CASES)
def test_statistic_is_fair_and_has_power(name):
    ref = _family(name)
    x = R.dist_weights(ref)
    cells = R.posterior_cells(ref, x)
    n = R.DIST_N * len(R.DIST_SEEDS)
    assert n == 1024
    for keys, prob, mult in cells:
        assert abs(prob.sum() - 1.0) <= 1e-12 and mult.sum() >= 1
    rng = np.random.default_rng(31)
    # the exact posterior passes
    x2, dof, impossible = R.chi_square(cells, R.draw_counts(cells, n, rng), n)
    print(name, "exact", x2, dof, R.bound(dof))
    assert dof >= 200
    assert impossible == 0 and x2 <= R.bound(dof)
    # uniform over each string's paths fails
    x2u, dofu, _ = R.chi_square(cells, R.draw_counts(cells, n, rng, lambda r, prob, mult: mult), n)
    print(name, "uniform", x2u, dofu)
    assert dofu == dof and x2u > R.bound(dof)
    # the posterior at other weights fails
    other = R.posterior_cells(ref, np.random.default_rng(R.DIST_WEIGHT_SEED + 1).normal(-1.0, 0.5, size=len(x)))
    x2o, dofo, _ = R.chi_square(cells, R.draw_counts(cells, n, rng, lambda r, prob, mult: other[r][1]), n)
    print(name, "other weights", x2o, dofo)
    assert dofo == dof and x2o > R.bound(dof)
