"""Device time of posterior path sampling on the dense path
(wfsa_dev_dense_sample_paths) at the c5 shape of test_dense_c5_4096_states
(4096 states, full transition matrix, 16 symbols, 4096 strings of at most 128
bytes) at n = 1, 16 and 64, split into its forward pass and its backward
kernel (device events: stats dense_sp_*_ms), beside one objective_grad call at
the same shape and weights (host clock around the call, which ends in a device
synchronise).  At 512 states, 16 symbols, 600 strings of at most 40 bytes also
the trellis tier's sample_paths (the same model loaded with WFSA_DENSE=0;
stats sample_path_ms) beside the dense call.  Medians of the repeats after a
warm-up call of each.  Writes profiles/dense_sample_paths/timing.json
(--out FILE); without a usable GPU the file says "not measured".  Run it under
a time limit of its own (timeout -k 10 SECONDS python
tools/time_dense_sample_paths.py ...).

  python tools/time_dense_sample_paths.py [--out FILE] [--repeat K] [--skip-c5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "w-fsa_amd"))

C5 = dict(n_states=4096, degree=1, vocab=16, emissions=16, dense=True, n_strings=4096, max_len=128, seed=2)
MID = dict(n_states=512, degree=1, vocab=16, emissions=16, dense=True, n_strings=600, max_len=40, seed=6)
SEED = 7


def _device(W, fsa, sym, off, wt, dense):
    os.environ["WFSA_DENSE"] = "1" if dense else "0"
    dev = W.Device(0)
    dev.load_model(fsa)
    dev.load_corpus(sym, off, wt / wt.sum())
    assert dev.stats()["dense"] == (1 if dense else 0)
    return dev


def _dense_call(dev, w, n, repeat):
    dev.dense_sample_paths(w, n, SEED)   # warm-up (allocates the history and the outputs)
    rows = []
    for _ in range(repeat):
        res = dev.dense_sample_paths(w, n, SEED)
        st = dev.stats()
        rows.append([st["sample_path_ms"], st["dense_sp_forward_ms"], st["dense_sp_backward_ms"]])
    med = np.median(np.array(rows), axis=0)
    srow, logw, prow, pidx, logq = res
    return dict(n=n, dense_sample_paths_ms=float(med[0]), forward_ms=float(med[1]), backward_ms=float(med[2]), all=rows,
                paths=int(len(logw)), path_entries=int(len(pidx)), finite=int(np.isfinite(logw).sum())), res


def measure_c5(W, repeat):
    syn = W.Synthetic(**C5)
    sym, off, wt = syn.corpus()
    fsa = W.Fsa.read_text(syn.wfsa_text)
    dev = _device(W, fsa, sym, off, wt, dense=True)
    dev.recognize()
    w = np.random.default_rng(11).normal(-8.5, 1.0, size=dev.n_params)
    st = dev.stats()
    out = dict(states=C5["n_states"], strings=int(len(wt)), symbols=int(off[-1]), rows=st["dense_rows"], steps=st["dense_steps"],
               np=st["dense_np"], engine=st["dense_blas"], repeat=repeat)
    _, _, logq = dev.objective_grad(w, want_logq=True)   # warm-up
    ev = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        dev.objective_grad(w, want_logq=False)
        ev.append(1e3 * (time.perf_counter() - t0))
    out["objective_grad_call_ms"] = float(np.median(ev))
    out["objective_grad_call_ms_all"] = ev
    out["calls"] = []
    for n in (1, 16, 64):
        d, res = _dense_call(dev, w, n, repeat)
        d["forward_over_objective_grad"] = d["forward_ms"] / out["objective_grad_call_ms"]
        d["logq_bytes_equal_objective_grad"] = bool(res[4].tobytes() == np.asarray(logq).tobytes())
        out["calls"].append(d)
        print(json.dumps(d), flush=True)
    return out


def measure_mid(W, repeat):
    syn = W.Synthetic(**MID)
    sym, off, wt = syn.corpus()
    fsa = W.Fsa.read_text(syn.wfsa_text)
    w = np.random.default_rng(3).normal(-6.0, 1.0, size=len(fsa.param_names()))
    dn = _device(W, fsa, sym, off, wt, dense=True)
    st = dn.stats()
    out = dict(states=MID["n_states"], strings=int(len(wt)), symbols=int(off[-1]), rows=st["dense_rows"], steps=st["dense_steps"],
               np=st["dense_np"], repeat=repeat, calls=[])
    got = {}
    for n in (1, 16, 64):
        d, got[n] = _dense_call(dn, w, n, repeat)
        out["calls"].append(d)
    try:
        sp = _device(W, fsa, sym, off, wt, dense=False)
        for d in out["calls"]:
            n = d["n"]
            ref = sp.sample_paths(w, n, SEED)   # warm-up
            tr = []
            for _ in range(repeat):
                sp.sample_paths(w, n, SEED)
                tr.append(sp.stats()["sample_path_ms"])
            d["trellis_sample_paths_ms"] = float(np.median(tr))
            d["trellis_sample_paths_ms_all"] = tr
            same = [np.array_equal(got[n][3][got[n][2][t]:got[n][2][t + 1]], ref[3][ref[2][t]:ref[2][t + 1]])
                    for t in range(len(ref[1]))] if np.array_equal(got[n][0], ref[0]) else []
            d["samples_equal_to_trellis"] = int(np.sum(same))
    except W.WfsaError as e:   # the trellis tier does not take the model
        out["trellis_error"] = str(e)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_sample_paths", "timing.json"))
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--skip-c5", action="store_true")
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    try:
        import wfsa_amd as W
        W.Device(0)
    except Exception as e:   # no library / no gfx950 device
        json.dump({"status": "not measured", "reason": str(e)}, open(args.out, "w"), indent=1)
        print("not measured:", e)
        return
    out = {"status": "measured",
           "clock": "dense_sample_paths and trellis sample_paths: device events around their kernels (stats sample_path_ms, "
                    "dense_sp_*_ms); objective_grad: host clock around the call, which ends in a device synchronise; medians of "
                    "the repeats after a warm-up"}
    out["mid512"] = measure_mid(W, args.repeat)
    print(json.dumps(out["mid512"]), flush=True)
    json.dump(out, open(args.out, "w"), indent=1)
    if not args.skip_c5:
        out["c5"] = measure_c5(W, args.repeat)
        json.dump(out, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
