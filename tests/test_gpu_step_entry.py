"""The step kernels' bits against the parent commit's, recorded.

Changes to how the step kernels wait and are scheduled (fb_kernels.hip
step_dot_kernel: the class-B small-bubble waves' priority; the loads at
entry tried with it) must move no result bit:

- tests/golden/step_entry/<shape>.npz, recorded on the GPU from the parent
  commit's library by tools/record_step_golden.py: the nine info rows of
  Init(7), Run(5), Run(4), x(), last_grad() and the KL of objective_grad()
  afterwards, on the default step path and with WFSA_QN_INKERNEL=1, the rmin
  column off and on -- compared byte for byte;
- a halted launch must store nothing, wherever its first loads are issued:
  the steps enqueued behind a halt leave x, the gradient and the next
  evaluation's KL as a learner that ran exactly to the halt has them.

"ambiguous" (4,479 class-A bubbles: 70 chunks, the last partial; 3,228
class-B bubbles in 28 structures, id 0 among them; multi-id waves; lane
groups on popular parameters) is the smallest corpus that takes every branch
of small_bubble.
"""
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "step_entry")

# two of test_gpu_ll_dot.py's shapes
SHAPES = {
    "A-small": dict(n_states=256, degree=8, vocab=64, emissions=1, n_strings=20_000, max_len=64, seed=1),
    "ambiguous": dict(n_states=256, degree=8, vocab=16, emissions=1, n_strings=8_000, max_len=64, seed=4,
                      compiled_only=True),
}
# name -> (WFSA_QN_INKERNEL or None: the cover rule decides, the rmin column)
SETTINGS = {
    "default": (None, False), "default_rmin": (None, True),
    "inkernel": ("1", False), "inkernel_rmin": ("1", True),
}

_corpora = {}
_golden = {}


@pytest.fixture(scope="module", autouse=True)
def _release_corpora():
    yield
    _corpora.clear()   # (the model handles go before the interpreter shuts down)


def _corpus(W, shape):
    """(fsa, sym, off, wt) of a shape, built once per session"""
    if shape in _corpora:
        return _corpora[shape]
    kw = dict(SHAPES[shape])
    compiled_only = kw.pop("compiled_only", False)
    syn = W.Synthetic(**kw)
    sym, off, wt = syn.corpus()
    fsa = W.Fsa.read_text(syn.wfsa_text)
    if compiled_only:   # the strings that compile, as test_gpu_ll_dot.py takes them
        dev = W.Device(0)
        dev.load_model(fsa)
        dev.load_corpus(sym, off, wt / wt.sum())
        dev.recognize()
        dev.objective_grad(np.full(len(fsa.param_names()), -1.0), want_logq=False)
        keep = np.flatnonzero(dev.string_tiers() < 0)
        lens = np.diff(off)[keep]
        off_k = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        sym = np.concatenate([sym[off[i]:off[i + 1]] for i in keep]).astype(np.uint8)
        off, wt = off_k, wt[keep]
    _corpora[shape] = (fsa, sym, off, wt)
    return _corpora[shape]


def _recorded(shape):
    if shape not in _golden:
        with np.load(os.path.join(GOLDEN, shape + ".npz")) as z:
            _golden[shape] = {k: z[k] for k in z.files}
    return _golden[shape]


def _learner(W, shape, monkeypatch, inkernel, rmin):
    if inkernel is None:
        monkeypatch.delenv("WFSA_QN_INKERNEL", raising=False)
    else:
        monkeypatch.setenv("WFSA_QN_INKERNEL", inkernel)
    lrn = W.QuasiNewtonLearner(0)
    lrn.set_info_rmin(rmin)
    lrn.BuildFromPacked(*_corpus(W, shape))
    lrn.Finalize()
    lrn.Init(7)
    return lrn


@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_step_bits_are_the_parent_commits(shape, setting, monkeypatch):
    import wfsa_amd as W
    inkernel, rmin = SETTINGS[setting]
    rec = _recorded(shape)
    lrn = _learner(W, shape, monkeypatch, inkernel, rmin)
    rows = np.array(lrn.Run(5, 1.0, -1.0) + lrn.Run(4, 1.0, -1.0), dtype=np.float64)
    if inkernel == "1" and not (rmin and shape == "ambiguous"):   # (there the bubbles outnumber the waves: not fused)
        assert lrn.stats()["qn_inkernel_waves"] > 0, "the in-kernel update did not run"
    assert lrn.stats()["ll_dot_launches"] > 0, "the stream-less launch did not run"
    x, grad = lrn.x(), lrn.last_grad()
    kl = np.array([lrn.objective_grad()[0]], dtype=np.float64)
    want = rec[f"{setting}.rows"]
    assert rows.shape == want.shape == (9, want.shape[1])
    bad = sorted(set(int(r) for r, _ in np.argwhere(rows.view(np.uint64) != want.view(np.uint64))))
    assert not bad, f"rows {bad} differ: {rows[bad].tolist()} vs {want[bad].tolist()}"
    assert rows.tobytes() == want.tobytes()
    assert x.tobytes() == rec[f"{setting}.x"].tobytes()
    assert grad.tobytes() == rec[f"{setting}.grad"].tobytes()
    assert kl.tobytes() == rec[f"{setting}.kl"].tobytes(), (kl, rec[f"{setting}.kl"])


@pytest.mark.parametrize("inkernel", [None, "1"], ids=["default", "inkernel"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_a_halted_launch_stores_nothing(shape, inkernel, monkeypatch):
    """the launches enqueued behind a halt return at once: nothing they could
    have stored shows"""
    import wfsa_amd as W
    a = _learner(W, shape, monkeypatch, inkernel, False)
    free = np.array(a.Run(10, 1.0, -1.0))   # a run that does not halt: its gradient-error column
    gerr = free[:, 1]
    assert gerr[2] < gerr[1], gerr
    tol = 0.5 * (gerr[1] + gerr[2])   # between rows 2 and 3
    # the finish halts at the first row whose gradient error and constraint
    # extremes are all within tol (qn_finish_compute): step 3, or the first
    # later one whose constraint columns have come down too
    within = (free[:, 1] <= tol) & (np.abs(free[:, 2]) <= tol) & (np.abs(free[:, 3]) <= tol)
    assert not within[:2].any() and within[2:6].any(), free[:, 1:4]
    h = int(np.flatnonzero(within)[0]) + 1
    b = _learner(W, shape, monkeypatch, inkernel, False)
    rows = b.Run(10, 1.0, tol)
    assert len(rows) == h, f"halted after {len(rows)} steps, not {h}: the later steps' rows were not reported skipped"
    c = _learner(W, shape, monkeypatch, inkernel, False)   # ran exactly to the halt and stopped
    rows_c = c.Run(h, 1.0, -1.0)
    assert np.array(rows).tobytes() == np.array(rows_c).tobytes() == free[:h].tobytes()
    assert b.x().tobytes() == c.x().tobytes()
    assert b.last_grad().tobytes() == c.last_grad().tobytes()
    kl_b, g_b, _ = b.objective_grad()
    kl_c, g_c, _ = c.objective_grad()
    assert np.float64(kl_b).tobytes() == np.float64(kl_c).tobytes()
    assert g_b.tobytes() == g_c.tobytes()
