"""Device time of the Viterbi decode on the dense path
(wfsa_dev_dense_best_paths) at the c5 shape of test_dense_c5_4096_states (4096
states, full transition matrix, 16 symbols, 4096 strings of at most 128
bytes), split into its table kernel, its T forward steps and its back-track
(device events: stats dense_bp_*_ms), beside one rmin() call at the same shape
and weights -- the (min, +) pass with the same tiling, the yardstick (host
clock around the call, which ends in a device synchronise).  At 512 states, 16
symbols, 600 strings of at most 40 bytes also the trellis tier's best_paths
(the same model loaded with WFSA_DENSE=0; stats best_path_ms) beside the dense
call.  Medians of the repeats after a warm-up call of each.  Writes
profiles/dense_best_paths/timing.json (--out FILE); without a usable GPU the
file says "not measured".  Run it under a time limit of its own
(timeout -k 10 SECONDS python tools/time_dense_best_paths.py ...).

  python tools/time_dense_best_paths.py [--out FILE] [--repeat K] [--skip-c5]
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


def _device(W, fsa, sym, off, wt, dense):
    os.environ["WFSA_DENSE"] = "1" if dense else "0"
    dev = W.Device(0)
    dev.load_model(fsa)
    dev.load_corpus(sym, off, wt / wt.sum())
    assert dev.stats()["dense"] == (1 if dense else 0)
    return dev


def _dense_call(dev, w, repeat):
    dev.dense_best_paths(w)   # warm-up (allocates the history)
    rows = []
    for _ in range(repeat):
        logw, prow, pidx = dev.dense_best_paths(w)
        st = dev.stats()
        rows.append([st["best_path_ms"], st["dense_bp_tables_ms"], st["dense_bp_forward_ms"], st["dense_bp_backtrack_ms"]])
    med = np.median(np.array(rows), axis=0)
    return dict(dense_best_paths_ms=float(med[0]), tables_ms=float(med[1]), forward_ms=float(med[2]),
                backtrack_ms=float(med[3]), all=rows, finite=int(np.isfinite(logw).sum()), path_entries=int(len(pidx))), (logw, prow, pidx)


def measure_c5(W, repeat):
    syn = W.Synthetic(**C5)
    sym, off, wt = syn.corpus()
    fsa = W.Fsa.read_text(syn.wfsa_text)
    dev = _device(W, fsa, sym, off, wt, dense=True)
    dev.recognize()
    w = np.random.default_rng(11).normal(-8.5, 1.0, size=dev.n_params)
    st = dev.stats()
    out = dict(states=C5["n_states"], strings=int(len(wt)), symbols=int(off[-1]), rows=st["dense_rows"], steps=st["dense_steps"],
               np=st["dense_np"], history_bytes=8 * st["dense_rows"] * st["dense_steps"] * st["dense_np"], repeat=repeat)
    dev.objective_grad(w, want_logq=False)
    dev.rmin()   # warm-up (allocates its buffers)
    rm = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        dev.rmin()
        rm.append(1e3 * (time.perf_counter() - t0))
    out["rmin_call_ms"] = float(np.median(rm))
    out["rmin_call_ms_all"] = rm
    d, _ = _dense_call(dev, w, repeat)
    out.update(d)
    out["forward_over_rmin"] = out["forward_ms"] / out["rmin_call_ms"]
    return out


def measure_mid(W, repeat):
    syn = W.Synthetic(**MID)
    sym, off, wt = syn.corpus()
    fsa = W.Fsa.read_text(syn.wfsa_text)
    w = np.random.default_rng(3).normal(-6.0, 1.0, size=len(fsa.param_names()))
    dn = _device(W, fsa, sym, off, wt, dense=True)
    st = dn.stats()
    out = dict(states=MID["n_states"], strings=int(len(wt)), symbols=int(off[-1]), rows=st["dense_rows"], steps=st["dense_steps"],
               np=st["dense_np"], repeat=repeat)
    d, got = _dense_call(dn, w, repeat)
    out.update(d)
    try:
        sp = _device(W, fsa, sym, off, wt, dense=False)
        ref = sp.best_paths(w)   # warm-up
        tr = []
        for _ in range(repeat):
            sp.best_paths(w)
            tr.append(sp.stats()["best_path_ms"])
        out["trellis_best_paths_ms"] = float(np.median(tr))
        out["trellis_best_paths_ms_all"] = tr
        out["same_paths_as_trellis"] = bool(np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]))
        out["same_logw_as_trellis"] = bool(got[0].tobytes() == ref[0].tobytes())
    except W.WfsaError as e:   # the trellis tier does not take the model
        out["trellis_best_paths_ms"] = None
        out["trellis_error"] = str(e)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_best_paths", "timing.json"))
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
           "clock": "dense_best_paths and trellis best_paths: device events around their kernels (stats best_path_ms, dense_bp_*_ms); "
                    "rmin: host clock around the call, which ends in a device synchronise; medians of the repeats after a warm-up"}
    out["mid512"] = measure_mid(W, args.repeat)
    print(json.dumps(out["mid512"]), flush=True)
    json.dump(out, open(args.out, "w"), indent=1)
    if not args.skip_c5:
        out["c5"] = measure_c5(W, args.repeat)
        print(json.dumps(out["c5"]), flush=True)
        json.dump(out, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
