"""Device time of unconditional generation (wfsa_dev_generate) at bench.py's c3
model, n = 1M samples of at most 128 bytes, beside posterior path sampling
(wfsa_dev_sample_paths, n = 1) over the c3 corpus on the same device: both from
device events (stats generate_ms / sample_path_ms), medians of the repeats
after a warm-up call of each, taken in alternation in one process.  Writes the
times, what the samples came to (bytes, path entries, status counts, the
longest walk) and the time per walk step to profiles/generate/timing.json
(--out FILE); without a usable GPU the file says "not measured".  Run it under
a time limit of its own (timeout -k 10 SECONDS python tools/time_generate.py ...).

  python tools/time_generate.py [--out FILE] [--repeat K] [--samples N] [--max-len L] [--strings-scale F]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "w-fsa_amd"))

# bench.py's c3 workload (max_len 128, seed 1)
C3 = dict(n_states=1024, degree=8, vocab=64, emissions=1, n_strings=1_000_000)


def measure(W, repeat, n, max_len, scale):
    spec = dict(C3, n_strings=max(1, int(C3["n_strings"] * scale)))
    syn = W.Synthetic(max_len=128, seed=1, **spec)
    sym, off, wt = syn.corpus()
    fsa = W.Fsa.read_text(syn.wfsa_text)
    dev = W.Device(0)
    dev.load_model(fsa)
    dev.load_corpus(sym, off, wt / wt.sum())
    dev.recognize()
    w = np.random.default_rng(0).normal(-1.5, 0.3, size=dev.n_params)
    dev.generate(w, n, max_len=max_len, seed=1)   # warm-up
    dev.sample_paths(w, 1, seed=1)
    gen, sp = [], []
    for r in range(repeat):
        got = dev.generate(w, n, max_len=max_len, seed=r)
        gen.append(dev.stats()["generate_ms"])
        dev.sample_paths(w, 1, seed=r)
        sp.append(dev.stats()["sample_path_ms"])
    g, q = float(np.median(gen)), float(np.median(sp))
    status = np.bincount(got["status"], minlength=3)
    # a walk of t transitions and e recorded emissions made t + e (+ 1 when truncated) choices; the single-member groups
    # carry no id, so the entries undercount them: the steps below are the walks' emissions, one per byte on c3 (1-byte emissions)
    steps = int(got["off"][-1])
    return dict(strings=int(len(wt)), samples=int(n), max_len=int(max_len), repeat=repeat, params=int(dev.n_params),
                generate_ms=g, generate_ms_all=gen, sample_paths_1_ms=q, sample_paths_1_ms_all=sp, ratio=g / q,
                bytes=int(got["off"][-1]), path_entries=int(got["prow"][-1]), complete=int(status[0]), truncated=int(status[1]),
                dead=int(status[2]), longest=int(np.diff(got["off"]).max()), mean_len=float(np.diff(got["off"]).mean()),
                ns_per_sample=1e6 * g / n, ns_per_emitted_byte_two_passes=1e6 * g / max(steps, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "generate", "timing.json"))
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--max-len", type=int, default=128)
    ap.add_argument("--strings-scale", type=float, default=1.0, help="fraction of c3's strings (sample_paths' side)")
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
           "clock": "device events (generate_ms: both walks, the running sums and the scan; sample_path_ms), median of the repeats, "
                    "calls in alternation"}
    out["c3"] = measure(W, args.repeat, args.samples, args.max_len, args.strings_scale)
    print(json.dumps(out["c3"]), flush=True)
    json.dump(out, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
