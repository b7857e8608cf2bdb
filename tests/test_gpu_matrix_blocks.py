"""GPU tests of matrix-file mode beyond one 256-thread block: the SpMV chain
(mp_logw_kernel, mp_string_kernel, mp_grad_kernel, mp_rmin_kernel) over
16,684 strings -- 65 full blocks, a 44-string tail, 66 partials, a second
round of mp_rmin_kernel's lanes, every wave of a block at work -- with a
permuted M, against the same chain in long double
(tests/matrix_blocks_cases.py; plain float64 stays within 2e-13 of it,
test_matrix_blocks_reference.py); the tie rule of min_pair at every level of
the rmin reduction (lanes, waves, blocks in both orientations, the strided loop);
load_paths' refusal of an M that does not name every path exactly once; and
the learners over matrix files written from a 59,380-path enumeration.
Needs a gfx950 device."""
import numpy as np
import pytest

import matrix_blocks_cases as M

pytestmark = pytest.mark.gpu


def _load(m):
    import wfsa_amd as W
    dev = W.Device(0)
    dev.load_paths(m["n"], m["prow"], m["pcol"], m["pdata"], m["mrow"], m["mcol"], m["p"])
    return dev


@pytest.mark.parametrize("plant", list(M.PLANTS))
def test_chain_over_66_blocks(plant):
    """LL and gradient to rtol 1e-12, log q to 1e-12 max(1, |log q|) (some
    strings have log q near 0), rmin's value to rtol 1e-12 and its path
    index exactly.  Two strings with identical path rows tie for the global
    minimum and the lower path index has to win; each plant puts them where
    one of the reduction's min_pair calls decides -- across blocks in both
    orientations, in the strided loop past 64 partials, across the waves of a
    block, across the lanes of a wave -- and where that call without its tie
    clause returns the higher index (matrix_blocks_cases.PLANTS; simulated in
    test_matrix_blocks_reference.py)"""
    m = M.synthetic(plant=plant)
    a, b, lower = m["plant"]
    dev = _load(m)
    rec, pc, used = dev.recognize()
    assert rec.all() and used.all()
    np.testing.assert_array_equal(pc, np.diff(m["mrow"]))
    lo = m["mcol"][m["mrow"][a if lower == "a" else b] + 1]
    for x in M.draws(m):
        ll, logq, grad, rpp = M.chain(m, x)
        got_ll, got_g, got_lq = dev.objective_grad(x)
        e_ll = abs(got_ll - ll) / abs(ll)
        e_lq = (np.abs(got_lq - logq) / np.maximum(1.0, np.abs(logq))).max()
        e_g = (np.abs(got_g - grad) / np.abs(grad)).max()
        want_v, want_i = M.rmin_of(m, rpp)
        v, i = dev.rmin()
        print("matrix_blocks %s LL %.2e logq %.2e grad %.2e rmin %.2e" % (plant, e_ll, e_lq, e_g, abs(v - want_v) / want_v))
        assert e_ll <= 1e-12 and e_lq <= 1e-12 and e_g <= 1e-12
        assert want_i == lo
        assert i == want_i and abs(v - want_v) <= 1e-12 * want_v, (v, i, want_v, want_i)
    # the same evaluation again: the same bytes
    a = dev.objective_grad(x)
    b = dev.objective_grad(x)
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


def test_single_path_corpus():
    """16,684 strings of one path each: no ambiguous string, rmin answers
    (0.0, -1), log q = P x in M's order"""
    m = M.synthetic(single=True)
    dev = _load(m)
    for x in M.draws(m)[:1]:
        ll, logq, grad, rpp = M.chain(m, x)
        assert (rpp == 1).all()
        got_ll, got_g, got_lq = dev.objective_grad(x)
        assert abs(got_ll - ll) <= 1e-12 * abs(ll)
        assert (np.abs(got_lq - logq) <= 1e-12 * np.maximum(1.0, np.abs(logq))).all()
        assert (np.abs(got_g - grad) <= 1e-12 * np.abs(grad)).all()
        assert dev.rmin() == (0.0, -1)


def test_load_paths_refuses_a_path_named_twice():
    """a path of two strings: one lane of mp_string_kernel would overwrite
    lw[l] while another still reads it"""
    import wfsa_amd as W
    prow, pcol, pdata = np.array([0, 1, 2, 3]), np.array([0, 1, 2]), np.ones(3)
    dev = W.Device(0)
    with pytest.raises(W.WfsaError, match="names path 1 twice") as e:
        dev.load_paths(3, prow, pcol, pdata, np.array([0, 2, 3]), np.array([0, 1, 1]), np.array([0.5, 0.5]))
    assert e.value.code == W._lib.WFSA_ERR_ARG


def test_load_paths_refuses_a_path_of_no_string():
    """a path no string names would keep its raw log weight as its gradient
    coefficient in mp_grad_kernel"""
    import wfsa_amd as W
    prow, pcol, pdata = np.array([0, 1, 2, 3]), np.array([0, 1, 2]), np.ones(3)
    dev = W.Device(0)
    with pytest.raises(W.WfsaError, match="M names 2 paths, P has 3") as e:
        dev.load_paths(3, prow, pcol, pdata, np.array([0, 1, 2]), np.array([0, 2]), np.array([0.5, 0.5]))
    assert e.value.code == W._lib.WFSA_ERR_ARG
    # and a good M still loads after the refusals
    dev.load_paths(3, prow, pcol, pdata, np.array([0, 2, 3]), np.array([2, 0, 1]), np.array([0.5, 0.5]))
    ll, g, lq = dev.objective_grad(np.array([-1.0, -2.0, -3.0]))
    np.testing.assert_allclose(lq, [np.log(np.exp(-3.0) + np.exp(-1.0)), -2.0], rtol=1e-14)


def _rmin_indices_ok(rpps, got):
    """the rmin column's path index, epoch by epoch, against the
    restatement's relative path probabilities.  Where the smallest one is
    isolated the index is the restatement's arg-min.  At the uniform start
    many of one string's 3,412 paths have the same weight, and which of
    them a float64 evaluation finds smallest is its rounding's choice (the
    device sums a path's weights in P's column order, numpy in BLAS's):
    there the index must name a path within 1e-12 (relative, the project's
    parity figure) of the minimum.  Returns which epochs were isolated"""
    isolated = []
    for rpp, i in zip(rpps, np.asarray(got, dtype=np.int64)):
        assert rpp[i] <= rpp.min() * (1 + 1e-12), (i, rpp[i], rpp.min())
        isolated.append(M.isolated_minimum(rpp))
        if isolated[-1]:
            assert i == int(np.argmin(rpp))
    return isolated


@pytest.fixture(scope="module")
def n20(tmp_path_factory):
    """the family's enumeration (59,380 paths over 300 strings: two string
    blocks, 232 path blocks), the dense restatement and its matrix files"""
    from matrix_io import write_matrices
    o, h = M.n20()
    prefix = str(tmp_path_factory.mktemp("n20") / "m")
    write_matrices(o, prefix)
    return o, h, prefix


def test_quasinewton_over_two_string_blocks(n20):
    """6 QN steps over the loaded matrices == the oracle's, the rmin column
    with the reference's path index (test_gpu_matrix.py's tolerances)"""
    import wfsa_amd as W
    o, h, prefix = n20
    o.qn_init(7)
    want, rmin, rpps = [], [], []
    for _ in range(6):
        h.x = o.x()
        _, rpp = h.modeled()
        rpps.append(rpp)
        i = int(np.argmin(rpp))
        rmin.append((rpp[i], float(i)))
        want.append(o.qn_step(1.0))
        assert not o.qn_halt(1e-6)
    lrn = W.QuasiNewtonLearner(0, optimizer="QuasiNewton")
    lrn.LoadMatrices(prefix)
    lrn.Finalize()
    rows = np.array(lrn.run(flags=7, epochs=6, tol=1e-6))
    want = np.array(want)
    assert rows.shape[0] == want.shape[0] == 6
    np.testing.assert_allclose(rows[:, 0], want[:, 0], rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(rows[:, 1:5], want[:, 1:5], rtol=1e-7, atol=1e-11)
    np.testing.assert_allclose(rows[:, 5], [r[0] for r in rmin], rtol=1e-9)
    assert _rmin_indices_ok(rpps, rows[:, 6]) == [False] + [True] * 5     # tied paths at the uniform start only


def test_hessian_over_two_string_blocks(n20):
    """3 HessianLearner epochs (H_f from 59,380 paths on the device) against
    the dense restatement, at test_hessian_from_matrix_files' tolerances.
    Damped steps (eta = 0.05): with full Newton steps this family's iterates
    leave every sensible range (|x| reaches 58 after one step and 3e14 after
    two, and the restatement stops with "Unable to continue!" in the third),
    so the epochs would compare two factorisations' rounding on a singular
    system; at eta = 0.05 |x| stays below 6 and the KKT matrix's smallest
    eigenvalue above 1e-5 of its largest (all of it asserted on the CPU,
    test_matrix_blocks_reference.py)"""
    import wfsa_amd as W
    o, h, prefix = n20
    h.init(31)
    want, rpps = [], []
    for _ in range(3):
        rpps.append(h.modeled()[1])
        want.append(h.step(M.N20_ETA))
    want = np.array(want)
    assert not h.degenerate
    lrn = W.HessianLearner(0)
    lrn.LoadMatrices(prefix)
    lrn.Finalize()
    lrn.Init(31)
    got = np.array(lrn.Run(3, eta=M.N20_ETA, tol=1e-6))
    assert got.shape == want.shape == (3, 9)
    np.testing.assert_allclose(got[:, 0], want[:, 0], rtol=1e-9, atol=1e-12)
    np.testing.assert_array_equal(got[:, 4:6], want[:, 4:6])
    np.testing.assert_allclose(got[:, 7], want[:, 7], rtol=1e-8, atol=1e-300)
    assert _rmin_indices_ok(rpps, got[:, 8]) == [False, True, True]   # the reference's path index
