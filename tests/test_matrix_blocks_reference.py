"""CPU checks of the multi-block matrix-file-mode input
(tests/matrix_blocks_cases.py): its shape is the one the GPU tests count on,
plain float64 in the opposite summation order stays within 2e-13 of the
long-double chain (five times inside the device's 1e-12), every planted tie
is the unique global minimum placed where a reduction without min_pair's tie
clause gets it wrong, and why the 59,380-path family's Hessian epochs are
damped."""
import numpy as np
import pytest

import matrix_blocks_cases as M


def test_shape():
    m = M.synthetic()
    S = len(m["mrow"]) - 1
    per = np.diff(m["mrow"])
    assert S == 16684 == 65 * 256 + 44 and m["n"] == 700
    assert sorted(per[per > 8]) == [64, 65, 256, 257, 300, 823] and per.min() == 1
    assert 0.3 < (per == 1).mean() < 0.45
    n_paths = len(m["prow"]) - 1
    assert 55000 < n_paths < 63000 and 1.1e6 < m["prow"][-1] < 1.3e6
    assert np.array_equal(np.sort(m["mcol"]), np.arange(n_paths)) and not np.array_equal(m["mcol"], np.arange(n_paths))
    assert 60000 < np.bincount(m["pcol"]).max() < 80000
    rows = np.diff(m["prow"])
    assert rows.min() == 1 and rows.max() == 40 and set(np.unique(m["pdata"])) == {1.0, 2.0, 3.0, 6.0}     # 6: the planted pair
    one = M.synthetic(single=True)
    assert (np.diff(one["mrow"]) == 1).all() and len(one["mrow"]) - 1 == S


def test_float64_chain_within_2e13():
    m = M.synthetic()
    for x in M.draws(m):
        ll, logq, grad, rpp = M.chain(m, x)
        ll2, logq2, grad2, rpp2 = M.chain(m, x, dtype=np.float64, reverse=True)
        gaps = (abs(ll2 - ll) / abs(ll), (np.abs(logq2 - logq) / np.maximum(1.0, np.abs(logq))).max(),
                (np.abs(grad2 - grad) / np.abs(grad)).max())
        print("float64 vs long double: LL %.1e, log q %.1e, gradient %.1e" % tuple(float(g) for g in gaps))
        assert max(gaps) <= 2e-13


@pytest.mark.parametrize("plant", list(M.PLANTS))
def test_planted_tie_needs_the_tie_rule(plant):
    """the planted pair ties exactly, is the unique global minimum, sits
    where its comment says -- and the device's reduction order without
    min_pair's tie clause returns the higher index of the two, so the GPU
    test of this plant fails if the clause goes"""
    m = M.synthetic(plant=plant)
    a, b, lower = M.PLANTS[plant]
    mrow, mcol = m["mrow"], m["mcol"]
    ka, kb = mrow[a] + 1, mrow[b] + 1          # the improbable path of each, in M order
    lo, hi = (mcol[ka], mcol[kb]) if lower == "a" else (mcol[kb], mcol[ka])
    assert lo < hi
    where = {"blocks4+61": (a // 256, b // 256) == (4, 61), "blocks3+60": (a // 256, b // 256) == (3, 60),
             "blocks1+65": (a // 256, b // 256) == (1, 65) and b < M.N_STRINGS,
             "waves0+2": a // 256 == b // 256 and (a % 256 // 64, b % 256 // 64) == (0, 2),
             "lanes8+13": a // 64 == b // 64 and (a % 64, b % 64) == (8, 13)}
    assert where[plant]
    amb = np.zeros(len(mcol), dtype=bool)
    amb[mcol] = np.repeat(np.diff(mrow) > 1, np.diff(mrow))
    others = amb.copy()
    others[[lo, hi]] = False
    for x in M.draws(m):
        for dtype in (np.longdouble, np.float64):      # identical rows, identical arithmetic: a tie in either
            rpp = M.chain(m, x, dtype=dtype)[3]
            assert rpp[lo] == rpp[hi]
            assert rpp[others].min() > 2 * rpp[lo]     # no other path comes near: rounding cannot reorder them
            assert M.rmin_of(m, rpp)[1] == lo
        assert M.simulate_rmin(m, rpp, tie_rule=True) == (float(rpp[lo]), lo)
        assert M.simulate_rmin(m, rpp, tie_rule=False) == (float(rpp[lo]), hi)


def test_n20_full_newton_steps_diverge_damped_ones_do_not():
    """why test_gpu_matrix_blocks.py's Hessian epochs over the 59,380-path
    family take steps of eta = 0.05 and not HessianOracle.run's full ones:
    at eta = 1 the first step takes |x| past 50, the second past 1e14 and the
    third epoch ends with "Unable to continue!" -- iterates that compare two
    factorisations' rounding, not the kernels.  At eta = 0.05 three epochs
    keep |x| below 6 and the KKT matrix's smallest eigenvalue above 1e-5 of
    its largest, and only the uniform start has tied smallest paths"""
    from oracle.oracle import OracleError
    o, h = M.n20()
    h.init(31)
    h.step(1.0)
    assert np.abs(h.x).max() > 50
    h.step(1.0)
    assert np.abs(h.x).max() > 1e14
    with pytest.raises(OracleError, match="Unable to continue"):
        h.run(flags=31, epochs=3, eta=1.0, tol=1e-6)
    h.init(31)
    isolated = []
    for _ in range(3):
        _, rpp = h.modeled()
        isolated.append(M.isolated_minimum(rpp))
        K, _ = h.kkt(h.grad(rpp), h.hf(rpp))
        ev = np.abs(np.linalg.eigvalsh(K))
        assert ev.min() > 1e-5 * ev.max()
        h.step(M.N20_ETA)
        assert not h.degenerate and np.abs(h.x).max() < 6
    assert isolated == [False, True, True]
    # the QuasiNewton run of the same test: tied paths at the start only
    o.qn_init(7)
    isolated = []
    for _ in range(6):
        h.x = o.x()
        isolated.append(M.isolated_minimum(h.modeled()[1]))
        o.qn_step(1.0)
    assert isolated == [False] + [True] * 5
