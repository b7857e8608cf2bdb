"""Device time of posterior path sampling (wfsa_dev_sample_paths) at n = 1, 16
and 64 beside the Viterbi decode (wfsa_dev_best_paths) and the K-best decode
at k = 16 on the same loaded corpus, for bench.py's c3 and famB shapes: all
from device events (stats sample_path_ms / best_path_ms / kbest_path_ms),
medians of the repeats after a warm-up call of each, taken in alternation in
one process.  Writes the times, their ratios to best_paths and best_paths' own
run-to-run spread to profiles/sample_paths/timing.json (--out FILE); without a
usable GPU the file says "not measured".  Run it under a time limit of its own
(timeout -k 10 SECONDS python tools/time_sample_paths.py ...).

  python tools/time_sample_paths.py [--out FILE] [--repeat K] [--strings-scale F]
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
NS = (1, 16, 64)
KBEST = 16


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
    st = dev.stats()
    out = dict(strings=int(len(wt)), total_symbols=int(off[-1]), nodes=st["n_nodes"], edges=st["n_edges"], repeat=repeat, n={})
    best_all, kbest_all = [], []
    for n in NS:
        dev.best_paths(w)   # warm-up
        dev.kbest_paths(w, KBEST)
        dev.sample_paths(w, n, seed=1)
        bp, kb, sp = [], [], []
        for r in range(repeat):
            dev.best_paths(w)
            bp.append(dev.stats()["best_path_ms"])
            dev.kbest_paths(w, KBEST)
            kb.append(dev.stats()["kbest_path_ms"])
            srow, _, prow, _, _ = dev.sample_paths(w, n, seed=r)
            sp.append(dev.stats()["sample_path_ms"])
        b, q = float(np.median(bp)), float(np.median(sp))
        best_all += bp
        kbest_all += kb
        out["n"][str(n)] = dict(paths=int(srow[-1]), path_entries=int(prow[-1]), best_paths_ms=b, sample_paths_ms=q,
                                ratio=q / b, best_paths_ms_all=bp, sample_paths_ms_all=sp)
    out["best_paths_ms"] = float(np.median(best_all))
    out["kbest16_paths_ms"] = float(np.median(kbest_all))
    out["kbest16_ratio"] = out["kbest16_paths_ms"] / out["best_paths_ms"]
    # the yardstick's own run-to-run spread: (max - min) / median over all its calls here
    out["best_paths_spread"] = float((max(best_all) - min(best_all)) / np.median(best_all))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_paths", "timing.json"))
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
    out = {"status": "measured", "strings_scale": args.strings_scale,
           "clock": "device events (sample_path_ms; best_path_ms; kbest_path_ms), median of the repeats, calls in alternation",
           "shapes": {}}
    for name, shape in SHAPES.items():
        out["shapes"][name] = measure(W, shape, args.repeat, args.strings_scale)
        print(name, json.dumps(out["shapes"][name]), flush=True)
        json.dump(out, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
