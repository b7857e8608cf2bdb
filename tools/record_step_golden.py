"""Records tests/golden/step_entry/<shape>.npz: the step kernels' bits before
the class-B waves' priority change (and the loads at entry tried with it),
from the library of parent commit 9408fc0 ("Hand-built bubble tests: class
bounds, size limits, lane groups").

tests/test_gpu_step_entry.py compares the current library against these
files byte for byte.  Build the parent's library beside the tree's and run

    WFSA_LIB=<parent>/libwfsa_amd.so python tools/record_step_golden.py [OUT_DIR]

on the GPU.  Each file holds, for the four settings (the default step path
and WFSA_QN_INKERNEL=1, the rmin column off and on): the nine info rows of
Init(7), Run(5), Run(4) (odd and even lengths: both weight parities), x(),
last_grad() and the KL of an objective_grad() afterwards.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "w-fsa_amd"))

PARENT = "9408fc0"

# two of tests/test_gpu_ll_dot.py's shapes
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


def corpus(W, shape):
    kw = dict(SHAPES[shape])
    compiled_only = kw.pop("compiled_only", False)
    syn = W.Synthetic(**kw)
    sym, off, wt = syn.corpus()
    fsa = W.Fsa.read_text(syn.wfsa_text)
    if compiled_only:   # the strings that compile, as tests/test_gpu_ll_dot.py takes them
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
    return fsa, sym, off, wt


def learner(W, corp, inkernel, rmin):
    if inkernel is None:
        os.environ.pop("WFSA_QN_INKERNEL", None)
    else:
        os.environ["WFSA_QN_INKERNEL"] = inkernel
    lrn = W.QuasiNewtonLearner(0)
    lrn.set_info_rmin(rmin)
    lrn.BuildFromPacked(*corp)
    lrn.Finalize()
    lrn.Init(7)
    return lrn


def trajectory(W, corp, inkernel, rmin):
    lrn = learner(W, corp, inkernel, rmin)
    rows = np.array(lrn.Run(5, 1.0, -1.0) + lrn.Run(4, 1.0, -1.0), dtype=np.float64)
    x, grad = lrn.x(), lrn.last_grad()
    kl = lrn.objective_grad()[0]
    return dict(rows=rows, x=x, grad=grad, kl=np.array([kl], dtype=np.float64))


def main():
    import wfsa_amd as W
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "step_entry")
    os.makedirs(out, exist_ok=True)
    for shape in SHAPES:
        corp = corpus(W, shape)
        rec = {"parent": np.array(PARENT)}
        for name, (inkernel, rmin) in SETTINGS.items():
            for k, v in trajectory(W, corp, inkernel, rmin).items():
                rec[f"{name}.{k}"] = v
            r = rec[f"{name}.rows"]
            assert r.shape[0] == 9 and np.isfinite(r).all(), (shape, name, r.shape)
            print(f"{shape} {name}: KL {r[0, 0]!r} -> {r[-1, 0]!r}, graderr {r[:, 1].tolist()}", flush=True)
        np.savez_compressed(os.path.join(out, shape + ".npz"), **rec)
        print(f"{shape}: {os.path.getsize(os.path.join(out, shape + '.npz'))} bytes", flush=True)


if __name__ == "__main__":
    main()
