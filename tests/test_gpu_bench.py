"""bench.py as a program: a plain run times exactly --steps steps, prints the
headline record alone (what --full adds stays out), and --dump-outputs
writes the last timed step's info row, weights and gradient -- the same
values a caller running the same steps in-process holds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

N, STEPS, WARMUP = 20_000, 3, 1


def test_plain_run_is_the_headline_alone_and_dumps_its_last_step(tmp_path):
    import wfsa_amd as W
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--strings-per-gpu", str(N),
                        "--steps", str(STEPS), "--warmup", str(WARMUP), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == STEPS and d["warmup"] == WARMUP and d["n_gpus"] == 1
    assert d["unit"] == "strings/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(d["config"]["global_strings"] / (d["ms_per_step"] * 1e-3), rel=1e-9)
    # what --full adds
    for k in ("info_rmin", "boundary", "cpu_baseline"):
        assert d[k] is None, k
    for k in ("dense_c5", "famB", "dense_c5_rocblas", "ll_rel_err_vs_reference_algorithm"):
        assert k not in d, k
    assert sorted(os.listdir(out)) == ["grad.npy", "info_row.npy", "x.npy"]
    got = {k: np.load(out / (k + ".npy")) for k in ("grad", "info_row", "x")}
    assert all(a.dtype == np.float64 and np.isfinite(a).all() for a in got.values())
    # the same steps in-process (the headline workload's automaton, --seed 1, --max-len 128)
    syn = W.Synthetic(n_states=1024, degree=8, vocab=64, emissions=1, n_strings=N, max_len=128, seed=1)
    sym, off, wt = syn.corpus()
    lrn = W.QuasiNewtonLearner(0)
    lrn.BuildFromPacked(W.Fsa.read_text(syn.wfsa_text), sym, off, wt)
    lrn.Finalize()
    lrn.Init(7)
    lrn.set_info_rmin(False)
    lrn.Run(WARMUP, 1.0, -1.0)
    rows = lrn.Run(STEPS, 1.0, -1.0)
    assert len(rows) == STEPS and d["config"]["global_strings"] == lrn.info()["n_strings"]
    assert got["x"].shape == got["grad"].shape == (lrn.n,)
    np.testing.assert_allclose(got["info_row"], rows[-1][:5], rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(got["x"], lrn.x(), rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(got["grad"], lrn.last_grad(), rtol=1e-10, atol=1e-15)
