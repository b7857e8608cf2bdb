"""Every output array of the eight per-string entry points (best_paths,
kbest_paths, sample_paths, posterior_counts, byte_marginals and the three
dense_ ones), getter outputs included, for comparing two builds of the library
byte for byte, and the host wall-clock of one call of each.

  WFSA_LIB=.../libwfsa_amd.so python tools/dump_features.py dump DIR
  python tools/dump_features.py compare DIR_A DIR_B      (one line per array)
  WFSA_LIB=.../libwfsa_amd.so python tools/dump_features.py time [--large]

dump and time load dense16 and auto128 (tests/dense_decode_reference.py), each
under WFSA_DENSE=1 and =0, at case_weights; time --large adds time_best_paths'
famB corpus on the trellis tiers and time_dense_best_paths' 512-state one on the
dense path.  time prints, per load and call, the median wall-clock of REPS
calls (each ends in a device synchronise) and the feature's *_ms stats field.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "w-fsa_amd"), os.path.join(ROOT, "tests")]
REPS = 7
LARGE = {0: dict(n_states=1024, degree=8, vocab=16, emissions=4, n_strings=100_000, max_len=128, seed=1),
         1: dict(n_states=512, degree=1, vocab=16, emissions=16, dense=True, n_strings=600, max_len=40, seed=6)}


def calls(dev, w, dense):
    """name -> (call, its stats field)"""
    if dense:
        bm = dev.dense_byte_marginals
        c = {"dense_best_paths": (lambda: dev.dense_best_paths(w), "best_path_ms")}
        c.update({"dense_sample_paths_n%d" % n: (lambda n=n: dev.dense_sample_paths(w, n, seed=7), "sample_path_ms") for n in (1, 16)})
        c.update({"dense_byte_marginals_rows%d_decode%d" % (r, d): (lambda r=r, d=d: bm(w, rows=bool(r), decode=bool(d)), "byte_marginal_ms")
                  for r, d in ((1, 0), (1, 1), (0, 1))})
        return c
    c = {"best_paths": (lambda: dev.best_paths(w), "best_path_ms")}
    c.update({"kbest_paths_k%d" % k: (lambda k=k: dev.kbest_paths(w, k), "kbest_path_ms") for k in (1, 4)})
    c.update({"sample_paths_n%d" % n: (lambda n=n: dev.sample_paths(w, n, seed=7), "sample_path_ms") for n in (1, 16)})
    c["posterior_counts"] = (lambda: dev.posterior_counts(w), "posterior_count_ms")
    c.update({"byte_marginals_decode%d" % d: (lambda d=d: dev.byte_marginals(w, decode=bool(d)), "byte_marginal_ms") for d in (0, 1)})
    return c


def loads(large):
    import wfsa_amd as W
    import dense_decode_reference as R
    for case in ("dense16", "auto128") + (("large",) if large else ()):
        for dense in (1, 0):
            os.environ["WFSA_DENSE"] = str(dense)
            if case == "large":
                syn = W.Synthetic(**LARGE[dense])
                text, (sym, off, wt) = syn.wfsa_text, syn.corpus()
            else:
                text, sym, off, wt = R.synthetic(case)
            fsa = W.Fsa.read_text(text)
            n_par = len(fsa.param_names())
            w = np.random.default_rng(0).normal(-1.5, 0.3, size=n_par) if case == "large" else R.case_weights(case, n_par)
            dev = W.Device(0)
            dev.load_model(fsa)
            dev.load_corpus(sym, off, wt / wt.sum())
            assert dev.stats()["dense"] == dense
            yield "%s_dense%d" % (case, dense), dev, calls(dev, w, dense)


def main():
    mode = sys.argv[1]
    if mode == "compare":
        a, b = sys.argv[2:4]
        names = sorted(set(os.listdir(a)) | set(os.listdir(b)))
        for n in names:
            both = os.path.exists(os.path.join(a, n)) and os.path.exists(os.path.join(b, n))
            same = both and open(os.path.join(a, n), "rb").read() == open(os.path.join(b, n), "rb").read()
            print(n, "identical" if same else "DIFFERENT" if both else "MISSING")
        return
    import wfsa_amd as W
    for load, dev, cs in loads("--large" in sys.argv):
        for name, (call, field) in cs.items():
            if mode == "dump":
                os.makedirs(sys.argv[2], exist_ok=True)
                for i, arr in enumerate(call()):
                    np.save(os.path.join(sys.argv[2], "%s.%s.%d.npy" % (load, name, i)), arr)
                continue
            try:
                call()   # warm-up
            except W.WfsaError as e:   # a capacity limit at this size is reported; any other error ends the run
                if e.code != W._lib.WFSA_ERR_CAPACITY:
                    raise
                print("%s %s refused: %s" % (load, name, e), flush=True)
                continue
            wall, ms = [], []
            for _ in range(REPS):
                t0 = time.perf_counter()
                call()
                wall.append((time.perf_counter() - t0) * 1e3)
                ms.append(dev.stats()[field])
            print("%s %s wall_ms %.4f %s %.4f" % (load, name, np.median(wall), field, np.median(ms)), flush=True)


if __name__ == "__main__":
    main()
