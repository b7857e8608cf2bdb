"""The two-kernel step's QN update as qn_wave_kernel (qn_kernel.hip): a wave
per constraint, no block barrier, instead of qn_step_kernel's block per
constraint.

WFSA_QN_WAVE=1 (the default) must give the bits of WFSA_QN_WAVE=0
(qn_step_kernel): the nine info rows of Init, Run(5), Run(4), x(),
last_grad() and the KL of the next objective_grad(), byte for byte; and
stats()["qn_wave_launches"] says which kernel ran.  The path rule
(wfsa_dev.hip enqueue_qn_step) takes the new kernel only when every
constraint fits one wave -- at most 64 members and 256 slot chunks -- the
rmin strings pass is not folded into the QN blocks and the update does not
ride in the stream kernel.

The hub automaton below is built by hand, in the style of bubble_gadgets.py:

    ^ -> H;  H emits x;  H -> d0, d1 (both emit a: the diamond), f_0 .. f_F-1
    (a letter of its own each), and $;  d_i -> H and $;  f_j -> H

H's constraint has F + 3 members when the corpus uses them all.  A string
x a x holds one class-A bubble whose four edges carry H -> d0, H -> d1,
d0 -> H and d1 -> H; the f_j make no bubble, so H -> f_j and H -> $ are
members without a slot chunk.  A string that ends in the diamond uses
d_i -> $, so the d_i's constraints have two members each: the smallest the
learner keeps (a constraint left with one used member is a fixed singleton,
trimmed away with it -- without such strings H's is the only constraint).  With
WFSA_SLOT_MERGE=0 every bubble edge has a slot of its own, so B bubbles give
H -> d0 and H -> d1 ceil(B / 16) chunks each: 2048 bubbles are 256 chunks in
H's constraint, 2049 are 258.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# test_gpu_step_entry.py's shapes and test_gpu_qn_inkernel.py's "mixed"
SHAPES = {
    "A-small": dict(n_states=256, degree=8, vocab=64, emissions=1, n_strings=20_000, max_len=64, seed=1),
    # 254 states: a constraint count that is no multiple of the four waves of a block
    "A-odd": dict(n_states=254, degree=8, vocab=64, emissions=1, n_strings=8_000, max_len=64, seed=1),
    # popular parameters: many chunks per member
    "ambiguous": dict(n_states=256, degree=8, vocab=16, emissions=1, n_strings=8_000, max_len=64, seed=4,
                      compiled_only=True),
    # the same with its traversal strings: the `out` term is live
    "mixed": dict(n_states=256, degree=8, vocab=16, emissions=1, n_strings=8_000, max_len=64, seed=4),
}
LETTERS = [c for c in "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz+-" if c not in "xa"]

_corpora = {}
_old = {}   # the WFSA_QN_WAVE=0 results, computed once per (case, flags, rmin)


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _corpora.clear()
    _old.clear()


def hub_text(fans):
    t = ["", "^", "$", "^  0", "^ H 0", "H x 0",
         "H d0 0 d1 0 " + " ".join(f"f{j} 0" for j in range(fans)) + " $ 0"]
    for d in ("d0", "d1"):
        t += [f"{d} a 0", f"{d} H 0 $ 0"]
    for j in range(fans):
        t += [f"f{j} {LETTERS[j]} 0", f"f{j} H 0"]
    return "\n".join(t) + "\n"


def hub_corpus(W, fans, bubbles, ends):
    """every f_j used; `bubbles` strings of one mid-string diamond each behind
    two fan visits (distinct strings), `ends` strings ending in the diamond"""
    assert fans <= len(LETTERS) and bubbles <= fans * fans and ends <= fans
    strings = [f"x{LETTERS[j]}x" for j in range(fans)] + ["x"]
    strings += [f"x{LETTERS[i % fans]}x{LETTERS[i // fans]}xax" for i in range(bubbles)]
    strings += [f"x{LETTERS[j]}xa" for j in range(ends)]
    assert len(set(strings)) == len(strings)
    raw = [s.encode() for s in strings]
    sym = np.frombuffer(b"".join(raw), dtype=np.uint8).copy()
    off = np.concatenate([[0], np.cumsum([len(s) for s in raw])]).astype(np.int64)
    wt = 1.0 + np.sqrt(np.arange(len(raw)) + 2.0)
    return W.Fsa.read_text(hub_text(fans)), sym, off, wt


def _corpus(W, case):
    if case in _corpora:
        return _corpora[case]
    if case.startswith("hub"):   # hub<members of H's constraint>_<mid-string diamonds>_<strings ending in one>
        members, bubbles, ends = (int(v) for v in case[3:].split("_"))
        _corpora[case] = hub_corpus(W, members - 3, bubbles, ends)
        return _corpora[case]
    kw = dict(SHAPES[case])
    compiled_only = kw.pop("compiled_only", False)
    syn = W.Synthetic(**kw)
    sym, off, wt = syn.corpus()
    fsa = W.Fsa.read_text(syn.wfsa_text)
    if compiled_only:   # the strings that compile, as test_gpu_step_entry.py takes them
        dev = W.Device(0)
        dev.load_model(fsa)
        dev.load_corpus(sym, off, wt / wt.sum())
        dev.recognize()
        dev.objective_grad(np.full(len(fsa.param_names()), -1.0), want_logq=False)
        keep = np.flatnonzero(dev.string_tiers() < 0)
        lens = np.diff(off)[keep]
        off_k = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        sym = np.concatenate([sym[off[i]:off[i + 1]] for i in keep]).astype(np.uint8)
        off, wt = off_k, wt[keep]
    _corpora[case] = (fsa, sym, off, wt)
    return _corpora[case]


def _learner(W, case, monkeypatch, wave, flags=7, rmin=False, inkernel=None, merge=True):
    monkeypatch.setenv("WFSA_QN_WAVE", wave)
    if inkernel is None:
        monkeypatch.delenv("WFSA_QN_INKERNEL", raising=False)
    else:
        monkeypatch.setenv("WFSA_QN_INKERNEL", inkernel)
    if merge:
        monkeypatch.delenv("WFSA_SLOT_MERGE", raising=False)
    else:
        monkeypatch.setenv("WFSA_SLOT_MERGE", "0")
    lrn = W.QuasiNewtonLearner(0)
    lrn.set_info_rmin(rmin)
    lrn.BuildFromPacked(*_corpus(W, case))
    lrn.Finalize()
    lrn.Init(flags)
    return lrn


def _trajectory(W, case, monkeypatch, wave, **kw):
    lrn = _learner(W, case, monkeypatch, wave, **kw)
    rows = np.array(lrn.Run(5, 1.0, -1.0) + lrn.Run(4, 1.0, -1.0), dtype=np.float64)
    st, info = lrn.stats(), lrn.info()
    x, grad = lrn.x(), lrn.last_grad()
    kl = np.array([lrn.objective_grad()[0]], dtype=np.float64)
    assert rows.shape[0] == 9 and np.isfinite(rows[:, :5]).all(), rows
    return dict(rows=rows, x=x, grad=grad, kl=kl, stats=st, info=info)


def _both(W, case, monkeypatch, **kw):
    """(new, old): the trajectories under WFSA_QN_WAVE=1 and =0, the second shared"""
    key = (case,) + tuple(sorted(kw.items()))
    if key not in _old:
        _old[key] = _trajectory(W, case, monkeypatch, "0", **kw)
        assert _old[key]["stats"]["qn_wave_launches"] == 0
    return _trajectory(W, case, monkeypatch, "1", **kw), _old[key]


def _same_bits(new, old):
    bad = sorted(set(int(r) for r, _ in np.argwhere(new["rows"].view(np.uint64) != old["rows"].view(np.uint64))))
    assert not bad, f"rows {bad} differ: {new['rows'][bad].tolist()} vs {old['rows'][bad].tolist()}"
    assert new["x"].tobytes() == old["x"].tobytes()
    assert new["grad"].tobytes() == old["grad"].tobytes()
    assert new["kl"].tobytes() == old["kl"].tobytes(), (new["kl"], old["kl"])


@pytest.mark.parametrize("flags", [7, 7 | 32], ids=["", "exp_lambda"])
@pytest.mark.parametrize("case", ["A-small", "A-odd", "ambiguous", "mixed"])
def test_wave_kernel_equals_qn_step_kernel(case, flags, monkeypatch):
    """(c) members of more than 8 chunks (ambiguous), (d) a partial last
    block (A-odd), (e) traversal strings (mixed), (g) both lambda updates"""
    import wfsa_amd as W
    new, old = _both(W, case, monkeypatch, flags=flags)
    print(case, "constraints", new["info"]["n_constraints"], "params", new["info"]["n_params"],
          "max group chunks", new["stats"]["max_group_chunks"], "fallback", new["stats"]["fallback_strings"])
    assert new["stats"]["qn_wave_launches"] == 9, "qn_wave_kernel did not run every step"
    assert new["stats"]["qn_inkernel_waves"] == 0
    if case == "A-odd":
        k = new["info"]["n_constraints"]
        assert k > 8 and k % 4 != 0, k
    if case == "ambiguous":   # some member alone has more than 8 chunks only if its constraint has
        assert new["stats"]["max_group_chunks"] > 8
    if case == "mixed":
        assert new["stats"]["fallback_strings"] > 0
    _same_bits(new, old)


def test_one_member_constraints_and_members_without_chunks(monkeypatch):
    """(a), (b), (d): the hub with 61 fans -- three constraints (one partial
    block) of 64, 2 and 2 members, two being the fewest a kept constraint
    has; 62 of H's members have no slot chunk"""
    import wfsa_amd as W
    new, old = _both(W, "hub64_200_4", monkeypatch)
    assert new["info"]["n_constraints"] == 3 and new["info"]["n_params"] == 68, new["info"]
    assert new["stats"]["small_bubbles_a"] == 204 and new["stats"]["fallback_strings"] == 0
    assert new["stats"]["qn_wave_launches"] == 9
    _same_bits(new, old)


@pytest.mark.parametrize("case,wave", [("hub64_200_4", True), ("hub65_200_4", False)])
def test_member_limit_of_the_path_rule(case, wave, monkeypatch):
    """(f) a constraint of exactly 64 members takes qn_wave_kernel, one of 65 qn_step_kernel"""
    import wfsa_amd as W
    new, old = _both(W, case, monkeypatch)
    members = int(case[3:5])
    assert new["info"]["n_params"] == members + 4, new["info"]
    assert new["stats"]["qn_wave_launches"] == (9 if wave else 0)
    _same_bits(new, old)


@pytest.mark.parametrize("case,chunks,wave", [("hub64_2048_0", 256, True), ("hub64_2049_0", 258, False)])
def test_chunk_limit_of_the_path_rule(case, chunks, wave, monkeypatch):
    """(f), (c) a slot per bubble edge: H's constraint, 64 members, has 256
    chunks (two members of 128: all four chunk rounds of a wave, 32 turns of
    the member sum) and takes qn_wave_kernel; with 258 it takes qn_step_kernel"""
    import wfsa_amd as W
    new, old = _both(W, case, monkeypatch, merge=False)
    assert new["stats"]["max_group_chunks"] == chunks, new["stats"]["max_group_chunks"]
    assert new["stats"]["qn_wave_launches"] == (9 if wave else 0)
    _same_bits(new, old)


def test_a_halted_run_equals_one_that_ran_to_the_halt(monkeypatch):
    """(h) the launches behind a halt store nothing and report skipped rows"""
    import wfsa_amd as W
    a = _learner(W, "A-small", monkeypatch, "1")
    free = np.array(a.Run(10, 1.0, -1.0))
    gerr = free[:, 1]
    assert gerr[2] < gerr[1], gerr
    tol = 0.5 * (gerr[1] + gerr[2])
    within = (free[:, 1] <= tol) & (np.abs(free[:, 2]) <= tol) & (np.abs(free[:, 3]) <= tol)
    assert not within[:2].any() and within[2:6].any(), free[:, 1:4]
    h = int(np.flatnonzero(within)[0]) + 1
    b = _learner(W, "A-small", monkeypatch, "1")
    rows = b.Run(10, 1.0, tol)
    assert len(rows) == h, f"halted after {len(rows)} steps, not {h}"
    assert b.stats()["qn_wave_launches"] >= h
    c = _learner(W, "A-small", monkeypatch, "1")   # ran exactly to the halt and stopped
    rows_c = c.Run(h, 1.0, -1.0)
    assert c.stats()["qn_wave_launches"] == h
    d = _learner(W, "A-small", monkeypatch, "0")   # the same through qn_step_kernel
    rows_d = d.Run(10, 1.0, tol)
    assert np.array(rows).tobytes() == np.array(rows_c).tobytes() == np.array(rows_d).tobytes() == free[:h].tobytes()
    assert b.x().tobytes() == c.x().tobytes() == d.x().tobytes()
    assert b.last_grad().tobytes() == c.last_grad().tobytes() == d.last_grad().tobytes()
    kl_b, g_b, _ = b.objective_grad()
    kl_c, g_c, _ = c.objective_grad()
    assert np.float64(kl_b).tobytes() == np.float64(kl_c).tobytes()
    assert g_b.tobytes() == g_c.tobytes()


@pytest.mark.parametrize("setting", ["rmin", "inkernel"])
def test_the_other_paths_are_unchanged(setting, monkeypatch):
    """(i) the rmin column folds its strings pass into qn_step_kernel's blocks,
    WFSA_QN_INKERNEL=1 runs the update in the stream kernel: no qn_wave_kernel"""
    import wfsa_amd as W
    kw = dict(rmin=True) if setting == "rmin" else dict(inkernel="1")
    new, old = _both(W, "A-small", monkeypatch, **kw)
    assert new["stats"]["qn_wave_launches"] == 0
    if setting == "inkernel":
        assert new["stats"]["qn_inkernel_waves"] > 0
    _same_bits(new, old)
