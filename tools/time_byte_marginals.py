"""Device time of the per-byte state posteriors (wfsa_dev_byte_marginals) without
and with the MEA decode, beside the Viterbi decode (wfsa_dev_best_paths) and the
posterior expected counts (wfsa_dev_posterior_counts, whose forward and backward
pass the marginals restate) on the same loaded corpus, for bench.py's c3 and famB
shapes: all from device events (stats byte_marginal_ms / best_path_ms /
posterior_count_ms), medians of the repeats after a warm-up call of each, taken
in alternation in one process.  Writes the times, the ratios to posterior_counts
and to best_paths, every call's run-to-run spread and the size of the dense
state-sum buffer to profiles/byte_marginals/timing.json (--out FILE); a shape
whose buffer is over the 4 GiB budget is recorded as refused, with its size;
without a usable GPU the file says "not measured".  Run it under a time limit of its own
(timeout -k 10 SECONDS python tools/time_byte_marginals.py ...).

  python tools/time_byte_marginals.py [--out FILE] [--repeat K] [--strings-scale F]
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


def groups_per_byte(fsa):
    """n_groups[c]: the states some transition leads to that have byte c in an
    emission -- the distinct owner states among the trellis destinations of c"""
    d = fsa.desc()
    n = d.n_states
    n_tr = d.tr_ptr[n]
    entered = {d.tr_dst[t] for t in range(n_tr)} - {d.end}
    out = np.zeros(256, dtype=np.int64)
    for u in entered:
        seen = set()
        for e in range(d.em_ptr[u], d.em_ptr[u + 1]):
            seen.update(d.em_bytes[d.em_off[e] + k] for k in range(d.em_len[e]))
        for c in seen:
            out[c] += 1
    return out


def mass_bytes(fsa, sym):
    """bytes of the dense state-sum buffer of a corpus: 8 per (corpus byte, group of that byte)"""
    return int(8 * (np.bincount(np.asarray(sym, dtype=np.uint8), minlength=256) * groups_per_byte(fsa)).sum())


def _marginals(W, dev, w, decode):
    """one call without copying the rows out; the kernels' device time and the entries"""
    n, m = C.c_int64(), C.c_int64()
    W.check_dev(W.load().wfsa_dev_byte_marginals(dev._h, w.ctypes.data_as(C.c_void_p), 1 if decode else 0, None, None, None, None,
                                                 C.byref(n), C.byref(m)))
    return dev.stats()["byte_marginal_ms"], n.value


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
               params=int(dev.n_params), repeat=repeat, mass_buffer_bytes=mass_bytes(fsa, sym))
    dev.best_paths(w)   # warm-up (the first posterior_counts call also sizes its output)
    dev.posterior_counts(w)
    dev.posterior_counts(w)
    try:
        _marginals(W, dev, w, False)
    except W.WfsaError as e:   # the dense state sums of this corpus are over the 4 GiB budget
        out["refused"] = str(e)
        return out
    _marginals(W, dev, w, True)
    bp, pc, bm, bd = [], [], [], []
    entries = 0
    for r in range(repeat):
        dev.best_paths(w)
        bp.append(dev.stats()["best_path_ms"])
        n = C.c_int64()
        W.check_dev(W.load().wfsa_dev_posterior_counts(dev._h, w.ctypes.data_as(C.c_void_p), None, None, C.byref(n)))
        pc.append(dev.stats()["posterior_count_ms"])
        ms, entries = _marginals(W, dev, w, False)
        bm.append(ms)
        bd.append(_marginals(W, dev, w, True)[0])
    b, p, m, d = (float(np.median(v)) for v in (bp, pc, bm, bd))
    out.update(mass_entries=int(entries), best_paths_ms=b, posterior_counts_ms=p, byte_marginals_ms=m, byte_marginals_decode_ms=d,
               decode_pass_ms=d - m, ratio_to_posterior_counts=m / p, decode_ratio_to_posterior_counts=d / p,
               ratio_to_best_paths=m / b, decode_ratio_to_best_paths=d / b,
               best_paths_spread=_spread(bp), posterior_counts_spread=_spread(pc), byte_marginals_spread=_spread(bm),
               byte_marginals_decode_spread=_spread(bd),
               best_paths_ms_all=bp, posterior_counts_ms_all=pc, byte_marginals_ms_all=bm, byte_marginals_decode_ms_all=bd)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "byte_marginals", "timing.json"))
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
           "clock": "device events (byte_marginal_ms; best_path_ms; posterior_count_ms), median of the repeats, calls in alternation",
           "shapes": {}}
    for name, shape in SHAPES.items():
        out["shapes"][name] = measure(W, shape, args.repeat, args.strings_scale)
        print(name, json.dumps(out["shapes"][name]), flush=True)
        json.dump(out, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
