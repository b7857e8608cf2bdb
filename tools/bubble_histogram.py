"""The small bubbles' structures per corpus: prepares each corpus with
WFSA_VERBOSE set, so the library prints per class the distinct structures
with their bubble counts and the waves holding 1 / 2 / 3+ structures
([bubble-shapes] lines on stderr), then the stats() counters of the
compiled-in structures.
Usage: python tools/bubble_histogram.py [c3|familyA|ambiguous|famB ...]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "w-fsa_amd"))
os.environ["WFSA_VERBOSE"] = "1"

CORPORA = {
    "c3": dict(n_states=1024, degree=8, vocab=64, emissions=1, n_strings=1_000_000, max_len=128, seed=1),
    "familyA": dict(n_states=1024, degree=8, vocab=64, emissions=1, n_strings=200_000, max_len=128, seed=1),
    "ambiguous": dict(n_states=256, degree=8, vocab=16, emissions=1, n_strings=8_000, max_len=64, seed=4),
    "famB": dict(n_states=1024, degree=8, vocab=16, emissions=4, n_strings=100_000, max_len=128, seed=1),
}


def main():
    import wfsa_amd as W
    for name in sys.argv[1:] or list(CORPORA):
        syn = W.Synthetic(**CORPORA[name])
        sym, off, wt = syn.corpus()
        fsa = W.Fsa.read_text(syn.wfsa_text)
        print(f"== {name}: {CORPORA[name]}", file=sys.stderr, flush=True)
        dev = W.Device(0)
        dev.load_model(fsa)
        dev.load_corpus(sym, off, wt / wt.sum())
        dev.recognize()
        dev.objective_grad(np.full(len(fsa.param_names()), -1.0), want_logq=False)
        st = dev.stats()
        print(f"== {name}: compiled strings {st['compiled_strings']}, bubbles {st['n_bubbles']} (small: class A "
              f"{st.get('small_bubbles_a')}, class B {st.get('small_bubbles_b')}), with a compiled-in "
              f"structure {st.get('shaped_bubbles')}, small-bubble waves with more than one structure id "
              f"{st.get('mixed_shape_waves')}", file=sys.stderr, flush=True)
        del dev


if __name__ == "__main__":
    main()
