"""Device time of the Viterbi decode (wfsa_dev_best_paths) against one
objective/gradient evaluation with log q on the same loaded corpus, for
bench.py's c3 and famB shapes: both from device events (stats best_path_ms /
last_call_ms), after a warm-up call of each.  Writes the times and their ratio
to profiles/best_paths/timing.json (--out FILE); without a usable GPU the file
says "not measured".

  python tools/time_best_paths.py [--out FILE] [--repeat K] [--strings-scale F]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "w-fsa_amd"))

# bench.py's WORKLOADS (max_len 128, seed 1)
SHAPES = {
    "c3": dict(n_states=1024, degree=8, vocab=64, emissions=1, n_strings=1_000_000),
    "famB": dict(n_states=1024, degree=8, vocab=16, emissions=4, n_strings=100_000),
}


def measure(W, shape, repeat, scale):
    spec = dict(shape, n_strings=max(1, int(shape["n_strings"] * scale)))
    syn = W.Synthetic(max_len=128, seed=1, **spec)
    sym, off, wt = syn.corpus()
    fsa = W.Fsa.read_text(syn.wfsa_text)
    dev = W.Device(0)
    dev.load_model(fsa)
    dev.load_corpus(sym, off, wt / wt.sum())
    dev.recognize()
    w = np.random.default_rng(0).normal(-1.5, 0.3, size=dev.n_params)
    dev.objective_grad(w, want_logq=True)   # warm-up
    dev.best_paths(w)
    ev, bp = [], []
    for _ in range(repeat):
        dev.objective_grad(w, want_logq=True)
        ev.append(dev.stats()["last_call_ms"])
        logw, prow, _ = dev.best_paths(w)
        bp.append(dev.stats()["best_path_ms"])
    st = dev.stats()
    e, b = float(np.median(ev)), float(np.median(bp))
    return dict(strings=int(len(wt)), total_symbols=int(off[-1]), nodes=st["n_nodes"], edges=st["n_edges"],
                compiled_strings=st["compiled_strings"], fallback_strings=st["fallback_strings"],
                path_entries=int(prow[-1]), decoded=int(np.isfinite(logw).sum()),
                objective_grad_logq_ms=e, best_paths_ms=b, ratio=b / e, repeat=repeat,
                objective_grad_logq_ms_all=ev, best_paths_ms_all=bp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "best_paths", "timing.json"))
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--strings-scale", type=float, default=1.0, help="fraction of each shape's strings")
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    try:
        import wfsa_amd as W
        W.Device(0)
    except Exception as e:   # no library / no gfx950 device
        json.dump({"status": "not measured", "reason": str(e)}, open(args.out, "w"), indent=1)
        print("not measured:", e)
        return
    out = {"status": "measured", "clock": "device events (best_path_ms; last_call_ms), median of the repeats",
           "shapes": {}}
    for name, shape in SHAPES.items():
        out["shapes"][name] = measure(W, shape, args.repeat, args.strings_scale)
        print(name, json.dumps(out["shapes"][name]), flush=True)
        json.dump(out, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
