"""Device time of posterior expected counts (wfsa_dev_posterior_counts) beside
the Viterbi decode (wfsa_dev_best_paths) and the sampler at n = 1
(wfsa_dev_sample_paths, which has the same forward pass) on the same loaded
corpus, for bench.py's c3 and famB shapes: all from device events (stats
posterior_count_ms / best_path_ms / sample_path_ms), medians of the repeats
after a warm-up call of each, taken in alternation in one process.  The split
of the kernel's time comes from its two timing-only variants
(WFSA_POSTERIOR_PHASES=1: the forward pass and log q alone; =2: no row scan),
timed in the same alternation: backward pass = phases 2 - phases 1, row scan =
full - phases 2.  Writes the times, the ratios to sample_paths(1) and to
best_paths and the comparison calls' own run-to-run spread to
profiles/posterior_counts/timing.json (--out FILE); without a usable GPU the
file says "not measured".  Run it under a time limit of its own
(timeout -k 10 SECONDS python tools/time_posterior_counts.py ...).

  python tools/time_posterior_counts.py [--out FILE] [--repeat K] [--strings-scale F]
"""
import argparse
import ctypes as C
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


def _spread(v):
    return float((max(v) - min(v)) / np.median(v))


def _posterior(W, dev, w, phases):
    """one call at the given phases (3: the real call); the kernel's device time"""
    if phases == 3:
        os.environ.pop("WFSA_POSTERIOR_PHASES", None)
    else:
        os.environ["WFSA_POSTERIOR_PHASES"] = str(phases)
    try:
        n = C.c_int64()
        W.check_dev(W.load().wfsa_dev_posterior_counts(dev._h, w.ctypes.data_as(C.c_void_p), None, None, C.byref(n)))
    finally:
        os.environ.pop("WFSA_POSTERIOR_PHASES", None)
    return dev.stats()["posterior_count_ms"], n.value


def measure(W, shape, repeat, scale):
    spec = dict(shape, n_strings=max(1, int(shape["n_strings"] * scale)))
    syn = W.Synthetic(max_len=128, seed=1, **spec)
    sym, off, wt = syn.corpus()
    fsa = W.Fsa.read_text(syn.wfsa_text)
    dev = W.Device(0)
    dev.load_model(fsa)
    dev.load_corpus(sym, off, wt / wt.sum())
    dev.recognize()
    w = np.ascontiguousarray(np.random.default_rng(0).normal(-1.5, 0.3, size=dev.n_params))
    st = dev.stats()
    out = dict(strings=int(len(wt)), total_symbols=int(off[-1]), nodes=st["n_nodes"], edges=st["n_edges"],
               params=int(dev.n_params), repeat=repeat)
    dev.best_paths(w)   # warm-up (the first posterior_counts call also sizes the output)
    dev.sample_paths(w, 1, seed=1)
    for ph in (3, 1, 2, 3):
        _posterior(W, dev, w, ph)
    bp, sp, pc = [], [], {1: [], 2: [], 3: []}
    entries = 0
    for r in range(repeat):
        dev.best_paths(w)
        bp.append(dev.stats()["best_path_ms"])
        dev.sample_paths(w, 1, seed=r)
        sp.append(dev.stats()["sample_path_ms"])
        for ph in (1, 2, 3):
            ms, n = _posterior(W, dev, w, ph)
            pc[ph].append(ms)
            entries = max(entries, n)
    b, q = float(np.median(bp)), float(np.median(sp))
    f, fb, full = (float(np.median(pc[ph])) for ph in (1, 2, 3))
    out.update(row_entries=int(entries), best_paths_ms=b, sample_paths1_ms=q, posterior_counts_ms=full,
               ratio_to_sample_paths1=full / q, ratio_to_best_paths=full / b,
               forward_ms=f, backward_ms=fb - f, row_scan_ms=full - fb,
               forward_share=f / full, backward_share=(fb - f) / full, row_scan_share=(full - fb) / full,
               best_paths_spread=_spread(bp), sample_paths1_spread=_spread(sp), posterior_counts_spread=_spread(pc[3]),
               best_paths_ms_all=bp, sample_paths1_ms_all=sp, forward_only_ms_all=pc[1], no_scan_ms_all=pc[2],
               posterior_counts_ms_all=pc[3])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posterior_counts", "timing.json"))
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
           "clock": "device events (posterior_count_ms; best_path_ms; sample_path_ms), median of the repeats, calls in alternation; "
                    "forward / backward / row scan from the timing-only variants WFSA_POSTERIOR_PHASES=1 / 2",
           "shapes": {}}
    for name, shape in SHAPES.items():
        out["shapes"][name] = measure(W, shape, args.repeat, args.strings_scale)
        print(name, json.dumps(out["shapes"][name]), flush=True)
        json.dump(out, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
