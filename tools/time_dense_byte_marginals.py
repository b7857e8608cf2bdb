"""Device time of the byte marginals and the MEA decode on the dense path
(wfsa_dev_dense_byte_marginals).  At 512 states, 16 symbols, 600 strings of at
most 40 bytes: the call with rows alone, with the decode alone and with both,
split into its four parts (device events: stats dense_bm_*_ms), beside the
trellis tier's byte_marginals with and without the decode (the same model
loaded with WFSA_DENSE=0; stats byte_marginal_ms).  At the c5 shape of
test_dense_c5_4096_states (4096 states, full transition matrix, 16 symbols,
4096 strings of at most 128 bytes): rows = 0, decode = 1 on the full corpus
beside one objective_grad call (host clock around the call, which ends in a
device synchronise) and one dense_best_paths call at the same weights; the
entries rows = 1 would need there; and, those being over 4 GiB, rows = 1 on
the largest prefix of the strings whose rows fit.  Medians of the repeats
after a warm-up call of each.  Writes profiles/dense_byte_marginals/timing.json
(--out FILE); without a usable GPU the file says "not measured".  Run it under
a time limit of its own (timeout -k 10 SECONDS python
tools/time_dense_byte_marginals.py ...).

  python tools/time_dense_byte_marginals.py [--out FILE] [--repeat K] [--skip-c5]
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
PARTS = ("byte_marginal_ms", "dense_bm_forward_ms", "dense_bm_backward_ms", "dense_bm_rows_ms", "dense_bm_decode_ms")
ROW_BUDGET = 4 << 30   # bytes of rows at 12 bytes an entry


def _device(W, fsa, sym, off, wt, dense):
    os.environ["WFSA_DENSE"] = "1" if dense else "0"
    dev = W.Device(0)
    dev.load_model(fsa)
    dev.load_corpus(sym, off, wt / wt.sum())
    assert dev.stats()["dense"] == (1 if dense else 0)
    return dev


def _dense_call(dev, w, rows, decode, repeat):
    dev.dense_byte_marginals(w, rows=rows, decode=decode)   # warm-up (allocates the history and the outputs)
    t = []
    for _ in range(repeat):
        res = dev.dense_byte_marginals(w, rows=rows, decode=decode)
        st = dev.stats()
        t.append([st[k] for k in PARTS])
    med = np.median(np.array(t), axis=0)
    d = dict(rows=int(rows), decode=int(decode), all=t, entries=int(len(res[1])), finite_logq=int(np.isfinite(res[4]).sum()))
    d.update({k: float(v) for k, v in zip(PARTS, med)})
    if decode:
        d.update(path_entries=int(len(res[8])), score_sum=float(np.nansum(res[5])))
    return d, res


def measure_mid(W, repeat):
    syn = W.Synthetic(**MID)
    sym, off, wt = syn.corpus()
    fsa = W.Fsa.read_text(syn.wfsa_text)
    w = np.random.default_rng(3).normal(-6.0, 1.0, size=len(fsa.param_names()))
    dn = _device(W, fsa, sym, off, wt, dense=True)
    st = dn.stats()
    out = dict(states=MID["n_states"], strings=int(len(wt)), symbols=int(off[-1]), rows=st["dense_rows"], steps=st["dense_steps"],
               np=st["dense_np"], repeat=repeat, calls=[])
    got = None
    for rows, decode in ((True, False), (False, True), (True, True)):
        d, got = _dense_call(dn, w, rows, decode, repeat)
        out["calls"].append(d)
    try:
        tr = _device(W, fsa, sym, off, wt, dense=False)
        for decode in (False, True):
            ref = tr.byte_marginals(w, decode=decode)   # warm-up
            t = []
            for _ in range(repeat):
                tr.byte_marginals(w, decode=decode)
                t.append(tr.stats()["byte_marginal_ms"])
            key = "trellis_byte_marginals_decode_ms" if decode else "trellis_byte_marginals_ms"
            out[key] = float(np.median(t))
            out[key + "_all"] = t
        out["trellis_entries"] = int(len(ref[1]))
        out["score_sum_trellis"] = float(np.nansum(ref[5]))
        out["largest_score_difference"] = float(np.nanmax(np.abs(ref[5] - got[5])))
    except W.WfsaError as e:   # the trellis tier does not take the model
        out["trellis_error"] = str(e)
    return out


def measure_c5(W, repeat, save):
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
    dev.dense_best_paths(w)   # warm-up
    bp = []
    for _ in range(repeat):
        best = dev.dense_best_paths(w)
        s = dev.stats()
        bp.append([s["best_path_ms"], s["dense_bp_forward_ms"]])
    out["dense_best_paths_ms"], out["dense_best_paths_forward_ms"] = (float(v) for v in np.median(np.array(bp), axis=0))
    d, res = _dense_call(dev, w, False, True, repeat)
    d["logq_bytes_equal_objective_grad"] = bool(res[4].tobytes() == np.asarray(logq).tobytes())
    d["forward_backward_over_objective_grad"] = (d["dense_bm_forward_ms"] + d["dense_bm_backward_ms"]) / out["objective_grad_call_ms"]
    d["decode_over_dense_best_paths_forward"] = d["dense_bm_decode_ms"] / out["dense_best_paths_forward_ms"]
    d["paths_equal_to_viterbi"] = int(sum(np.array_equal(res[8][res[7][s]:res[7][s + 1]], best[2][best[1][s]:best[1][s + 1]])
                                          for s in range(len(wt))))
    out["decode_alone"] = d
    print(json.dumps(d), flush=True)
    save(out)   # (the prefix run below allocates 4 GiB of rows: keep what is measured so far)
    del dev, res
    # rows = 1: every state emits every symbol here, so a byte lists up to n_states states
    per_byte = C5["n_states"]
    out["entries_needed_upper_bound"] = int(off[-1]) * per_byte
    out["row_bytes_needed_upper_bound"] = int(off[-1]) * per_byte * 12
    n = int(np.searchsorted(off, ROW_BUDGET // (12 * per_byte), side="right") - 1)
    out["prefix_strings"], out["prefix_symbols"] = n, int(off[n])
    sub = _device(W, fsa, sym[:off[n]], off[:n + 1], wt[:n], dense=True)
    s = sub.stats()
    out["prefix_rows"], out["prefix_steps"] = s["dense_rows"], s["dense_steps"]
    d, res = _dense_call(sub, w, True, True, repeat)
    d["entries_per_byte"] = d["entries"] / max(1, int(off[n]))
    out["rows_on_prefix"] = d
    print(json.dumps(d), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_byte_marginals", "timing.json"))
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
           "clock": "dense_byte_marginals, dense_best_paths and trellis byte_marginals: device events around their kernels (stats "
                    "byte_marginal_ms, dense_bm_*_ms, best_path_ms); objective_grad: host clock around the call, which ends in a "
                    "device synchronise; medians of the repeats after a warm-up"}
    out["mid512"] = measure_mid(W, args.repeat)
    print(json.dumps(out["mid512"]), flush=True)
    json.dump(out, open(args.out, "w"), indent=1)
    if not args.skip_c5:
        def save(c5):
            out["c5"] = c5
            json.dump(out, open(args.out, "w"), indent=1)

        save(measure_c5(W, args.repeat, save))


if __name__ == "__main__":
    main()
