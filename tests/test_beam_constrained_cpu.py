"""No GPU: what the constrained beam-search tests rest on.
(a) tests/beam_constrained_oracle.py with neutral constraints reproduces oracle/beam_np.beam_loop on beam_small_e3 / beam_small_e5.
(b) Every direct fixture keeps MARGIN between adjacent candidates of its top k + 1 and between the rank scores of an image, and its
    constraint is live; the edge scenarios do what their docstrings say.
(c) Hand-written cases of the n-gram rule.
(d) The ABI validation of set_beam_pick_constrained_f32 through the loaded library (no compute call), and the argument errors of
    evaluate.BeamConstraints / `constraints=`.
(e) The search fixture of tests/test_hip_beam_constrained_search.py on the golden models: near ties stay within the cap, and
    the unconstrained result of some image violates every constraint the GPU test turns on."""
import ctypes as C
import math

import numpy as np
import pytest

import beam_constrained_fixtures as F
import beam_constrained_oracle as BO
import beam_parity
from oracle import beam_np, cases, dcnet_np as DN, editnet_np as EN


# ---- (a)
def _np_search(states, V, start, end, k, c, max_steps=50):
    def step(words):
        return [s.step(words) for s in states]

    def reindex(rows):
        for s in states:
            s.reindex(np.asarray(rows))
    return BO.search(step, reindex, 1, k, V, start, end, c, max_steps)


def np_models(d, b, k, model):
    Pe, Pd = EN.cast_params(d["sd_e"]), DN.cast_params(d["sd_d"])
    one = (d["X"][b:b + 1], d["prev"][b:b + 1], d["plen"][b:b + 1])
    e, dn = beam_np.EditNetBeam(Pe, *one, k), beam_np.DcnetBeam(Pd, one[1], one[2], k)
    return {"editnet": [e], "dcnet": [dn], "ensemble": [e, dn]}[model], Pe["fc.weight"].shape[0]


@pytest.mark.parametrize("name", ["beam_small_e3", "beam_small_e5"])
def test_neutral_constraints_reproduce_beam_loop(name):
    d = cases.build_beam(name)
    wm, B = d["wm"], d["case"]["B"]
    start, end = wm["<start>"], wm["<end>"]
    Pe, Pd = EN.cast_params(d["sd_e"]), DN.cast_params(d["sd_d"])
    n = 0
    for k in d["beams"]:
        for b in range(B):
            one = (d["X"][b:b + 1], d["prev"][b:b + 1], d["plen"][b:b + 1])
            refs = {"editnet": lambda: beam_np.beam_editnet(Pe, *one, start, end, k),
                    "dcnet": lambda: beam_np.beam_dcnet(Pd, one[1], one[2], start, end, k),
                    "ensemble": lambda: beam_np.beam_ensemble(Pe, Pd, *one, start, end, k)}
            for model in ("editnet", "dcnet", "ensemble"):
                seq, score, margin = refs[model]()
                states, V = np_models(d, b, k, model)
                (tok, sc), = _np_search(states, V, start, end, k, BO.NEUTRAL)[0]
                if np.isnan(score):
                    assert np.isnan(sc) and tok[:4] == seq[:4], (name, k, b, model)
                    continue
                assert abs(sc - score) < beam_parity.SCORE_TOL, (name, k, b, model, sc, score)   # (beam_loop sums in float32)
                if margin > beam_parity.MARGIN_MIN:
                    assert tok == seq, (name, k, b, model, tok, seq)
                    n += 1
    assert n >= len(d["beams"]) * B * 2, n


# ---- (b)
def test_tolerance_and_gap():
    assert 0.0 < F.TOL < 1e-4 and F.GAP == 2 * F.TOL and F.MARGIN == 10 * F.GAP and F.NEAR_TIE_FRACTION == 0.02
    assert F.MARGIN <= 0.002                      # what the seeds were chosen with
    assert sorted(F.SEEDS) == F.DIRECT and len(F.DIRECT) == 40


@pytest.mark.parametrize("shape,cname,models", F.DIRECT)
def test_direct_fixtures_keep_their_margins_and_their_constraint_is_live(shape, cname, models):
    gap, rgap, live = F.direct_quality(shape, cname, models)
    print(shape, cname, models, "gap %.4f rank gap %.4f" % (gap, rgap), "live", live)
    assert gap >= F.MARGIN and rgap >= F.MARGIN and live
    ref = F.direct_reference(shape, cname, models)
    assert int(ref[-1][0]["n_done"].sum()) > 0                               # hypotheses complete inside the four steps
    c = F.CONSTRAINTS[cname]
    last = ref[-1][0]
    for i in range(last["n_done"].shape[0]):                                 # and what completed obeys the constraints
        for j in range(int(last["n_done"][i])):
            _obeys(last["done_seq"][i, j, :last["done_len"][i, j]].tolist(), c, F.END, first=F.L0)


def _obeys(seq, c, end, first=1):
    """the tokens from position `first` on (those the search chose) break no rule"""
    assert seq[-1] == end and len(seq) - 2 >= c.min_len, seq              # <start>, at least min_len words, <end>
    for p in range(first, len(seq)):
        assert seq[p] not in c.banned, (seq, p)
        assert seq[p] not in BO.ngram_words(seq[:p], c.no_repeat_ngram), (seq, p)


def test_edge_scenarios_do_what_they_say():
    t = F.edge_reference("ties")
    assert t[0][2].tolist() == [5, 6, 8] and t[0][4][0]["free_top"][1] == 4 and t[0][4][0]["live"]
    assert len({float(x) for x in t[0][0]["scores"][0]}) == 1
    assert t[1][2].tolist() == [9, 10, 9] and t[1][3].tolist() == [0, 0, 1]
    m = F.edge_reference("min_len")
    assert all(m[s][4][0]["free_top"][1] % F.EDGE_V == F.END and m[s][4][0]["live"] for s in (0, 1))
    assert m[0][0]["n_done"][0] == 0 and m[1][0]["n_done"][0] == 0 and m[2][0]["n_done"][0] >= 1
    assert (m[2][0]["done_len"][0, :m[2][0]["n_done"][0]] - 2 >= 2).all()
    f = F.edge_reference("few_none_finished")
    assert len(f[0][4][0]["top"]) == 2 and f[0][0]["k_left"][0] == 3 and np.isinf(f[0][0]["scores"][0, 2])    # fewer than k survivors
    assert f[1][4][0]["exhausted"] and f[1][0]["k_left"][0] == 0 and f[1][0]["best_len"][0] == 0              # no survivor
    assert np.isinf(f[1][0]["best_score"][0]) and f[1][3][:3].tolist() == [0, 1, 2] and f[2][4][0] is None
    assert f[0][0]["k_left"][1] == 2 and f[1][0]["k_left"][1] == 0 and f[2][4][1] is None                     # k_left < k, then finished
    assert f[2][4][2] is not None and f[2][0]["k_left"][2] == 3                                               # beside a live image
    a, plain = F.edge_reference("alpha_reversal"), F.edge_reference("alpha_reversal", True)
    assert a[2][0]["n_done"][0] == 2 and plain[2][0]["n_done"][0] == 2
    assert plain[2][0]["done_score"][0, 0] > plain[2][0]["done_score"][0, 1] + F.MARGIN                       # the sums say: the first
    assert a[2][0]["done_score"][0, 1] > a[2][0]["done_score"][0, 0] + F.MARGIN                               # the rank scores: the second
    assert plain[2][0]["best_len"][0] == 3 and a[2][0]["best_len"][0] == 4
    assert math.isclose(a[2][0]["done_score"][0, 1], (math.log(0.3) + math.log(0.9)) / 3 ** 0.7, rel_tol=1e-6)     # (float32 logits)


# ---- (c)
def test_ngram_rule_by_hand():
    S = 2                                                                  # <start>
    assert BO.ngram_words([S, 5, 6, 5], 1) == {5, 6}                       # n = 1: every word so far
    assert BO.ngram_words([S], 1) == set()                                 # nothing generated yet
    assert BO.ngram_words([S, S, 7], 1) == {S, 7}                          # position 0 never takes part, a later <start> does
    assert BO.ngram_words([S, 5, 6, 5], 2) == {6}                          # n = 2: what followed the last word before
    assert BO.ngram_words([S, 5, 6, 7], 2) == set()
    assert BO.ngram_words([S, 5], 2) == set() and BO.ngram_words([S], 2) == set()          # L - n < 1, L < n
    assert BO.ngram_words([S, 5, 5], 2) == {5}                             # a match at i = L - n (= 1), overlapping the suffix
    assert BO.ngram_words([S, S, 5, S], 2) == {5}                          # the bigram (S, 5) at i = 1; (s[0], s[1]) is not one
    assert BO.ngram_words([S, 5], 3) == set() and BO.ngram_words([S, 5, 6], 3) == set()    # L < n and L == n
    assert BO.ngram_words([S, 5, 6, 9, 5, 6], 3) == {9}                    # a match at i = 1
    assert BO.ngram_words([S, 8, 5, 6, 5, 6], 3) == {5}                    # a match at i = L - n = 3 (overlapping)
    assert BO.ngram_words([S, 5, 6, 9, 5, 6, 4, 5, 6], 3) == {9, 4}        # i = 1 and i = 4
    assert BO.ngram_words([S, 5, 6, 9, 6, 5], 3) == set()
    c = BO.Constraints(no_repeat_ngram=2, min_len=3, banned=(1,))
    assert BO.removed_words([S, 5, 6, 5], c, 3) == {1, 6} and BO.removed_words([S, 5, 6], c, 3) == {1, 3}
    assert BO.rank_score(-3.0, 4, 0.0) == -3.0 and BO.rank_score(-3.0, 4, 0.5) == -1.5


# ---- (d)
@pytest.fixture(scope="module")
def lib():
    from show_edit_tell_amd import _lib
    return _lib.load()


def test_abi_validation_before_any_hip_call(lib):
    from show_edit_tell_amd import _lib
    for name in ("set_beam_pick_constrained_f32", "set_beam_pick_constrained_workspace_bytes"):
        assert name in _lib.PROTOTYPES and name not in _lib.MISSING
    assert len(lib.set_beam_pick_constrained_f32.argtypes) == len(lib.set_beam_pick_nbest_f32.argtypes) + 3
    wsb = lib.set_beam_pick_constrained_workspace_bytes
    assert wsb(0, 3) == 0 and wsb(2, 0) == 0 and wsb(2, 9) == 0 and wsb(2, 3) >= 2 * 2 * 3 * 8 * 4 and wsb(2, 3) % 256 == 0
    one = C.c_void_p(16)                      # (never dereferenced: the checks come first)
    big = 1 << 20

    def call(k=3, V=100, ld=100, cur=1, Lmax=8, ws=one, ws_bytes=big, c="default", ds=one, nd=one, logits=one, n=0, min_len=0,
             alpha=0.0, n_banned=0, banned=None):
        cc = _lib.BeamConstraintsC(n, min_len, alpha, n_banned, banned) if c == "default" else c
        return lib.set_beam_pick_constrained_f32(logits, None, ld, 2, k, V, 99, cur, Lmax, one, one, one, one, one, one, one, one, one,
                                                 ds, one, one, nd, None if cc is None else C.byref(cc), ws, ws_bytes, None)
    ARG, UNS = 1, 2
    assert call(c=None) == ARG and call(ds=None) == ARG and call(nd=None) == ARG and call(logits=None) == ARG
    assert call(ws=None) == ARG and call(ws=C.c_void_p(24)) == ARG and call(ws_bytes=wsb(2, 3) - 1) == ARG
    assert call(n=-1) == ARG and call(n=17) == ARG and call(min_len=-1) == ARG
    assert call(alpha=-0.5) == ARG and call(alpha=float("nan")) == ARG and call(alpha=float("inf")) == ARG
    assert call(n_banned=-1, banned=one) == ARG and call(n_banned=65, banned=one) == ARG
    assert call(n_banned=2, banned=None) == ARG and call(n_banned=0, banned=one) == ARG
    assert call(cur=0) == ARG and call(cur=8) == ARG and call(ld=99) == ARG and call(V=0) == ARG      # set_beam_pick_f32's
    assert call(k=9) == UNS and call(Lmax=257, cur=5) == UNS and call(k=8, V=1 << 28, ld=1 << 28) == UNS


class _Vocab:
    vocab_size = 50


def test_beam_constraints_argument_errors():
    from show_edit_tell_amd import evaluate as ev
    wm = {"<start>": 2, "<end>": 3, "<unk>": 1, "<pad>": 0, "cat": 7}
    ok = ev.BeamConstraints(no_repeat_ngram=3, min_length=4, length_penalty=0.7, banned_words=("<unk>", 9))
    assert not ok.neutral() and ok.banned_ids(wm, 50) == [1, 9]
    assert ev.BeamConstraints().neutral() and ev.BeamConstraints(0, 0, 0.0, ()).neutral()
    assert ev._active(None) is None and ev._active(ev.BeamConstraints()) is None and ev._active(ok) is ok
    for kw in (dict(no_repeat_ngram=-1), dict(no_repeat_ngram=17), dict(no_repeat_ngram=1.5), dict(min_length=-1),
               dict(length_penalty=-0.1), dict(length_penalty=float("nan")), dict(length_penalty=float("inf")),
               dict(banned_words=range(65))):
        with pytest.raises(ValueError):
            ev.BeamConstraints(**kw)
    assert len(ev.BeamConstraints(banned_words=range(64)).banned_words) == 64
    for bad in (("dog",), (50,), (-1,), ("<end>",), (3,)):                  # unknown word, out of range, <end> by name and by id
        with pytest.raises(ValueError):
            ev.BeamConstraints(banned_words=bad).banned_ids(wm, 50)
    with pytest.raises(TypeError):
        ev._active({"no_repeat_ngram": 2})
    # every entry checks `constraints=` before it touches the model (here: none)
    bad = ev.BeamConstraints(banned_words=("dog",))
    m = _Vocab()
    for f, args in ((ev.beam_search_editnet, (m, None, None, None, wm)), (ev.beam_search_editnet_batched, (m, None, None, None, wm)),
                    (ev.beam_search_dcnet, (m, None, None, wm)), (ev.beam_search_dcnet_batched, (m, None, None, wm)),
                    (ev.beam_search_ensemble, (m, m, None, None, None, wm)), (ev.beam_search_ensemble_batched, (m, m, None, None, None, wm)),
                    (ev.beam_search_adaptive, (m, None, None, None, None, wm)), (ev.beam_search_adaptive_batched, (m, None, None, None, None, wm))):
        with pytest.raises(ValueError):
            f(*args, 3, constraints=bad)
        with pytest.raises(TypeError):
            f(*args, 3, constraints="no_repeat_ngram=2")


# ---- (e)
@pytest.mark.parametrize("model", ["editnet", "dcnet", "ensemble"])
def test_search_fixture_on_the_golden_models(model):
    """the oracle's constrained search on beam_small_e5's numpy models, the GPU test's images, beams and constraints: picks whose
    oracle margin is below GAP stay within NEAR_TIE_FRACTION of all picks; the results obey the constraints; and for at least one
    image the UNCONSTRAINED result breaks the rule (the precondition the GPU test asserts on the device, too)"""
    import nbest_oracle as NO
    d = dict(cases.build_beam(F.SEARCH_FIXTURE))
    d["sd_e"], d["sd_d"] = NO.shifted(d, F.SEARCH_SHIFT)
    wm = d["wm"]
    start, end = wm["<start>"], wm["<end>"]
    for cname, c in sorted(F.search_constraints(wm).items()):
        for k in F.SEARCH_BEAMS:
            picks = near = broken = 0
            for b in F.SEARCH_IMAGES:
                states, V = np_models(d, b, k, model)
                ans, nbest, steps = _np_search(states, V, start, end, k, c, F.SEARCH_MAX_STEPS)
                for info in steps:
                    if info[0]:
                        v = [x for x, _ in info[0]["top"]]
                        gaps = [p - q for p, q in zip(v, v[1:])][:info[0]["counted"]]
                        picks += len(gaps)
                        near += sum(1 for g in gaps if g < F.GAP)
                for seq, r in nbest[0]:
                    _obeys(seq, c, end)
                assert all(x[1] >= y[1] for x, y in zip(nbest[0], nbest[0][1:]))
                states, V = np_models(d, b, k, model)
                (free, _), = _np_search(states, V, start, end, k, BO.NEUTRAL, F.SEARCH_MAX_STEPS)[0]
                broken += F.violates(free, c, end)
            print(model, cname, k, "picks", picks, "near ties", near, "unconstrained results that break the rule", broken)
            assert near <= F.NEAR_TIE_FRACTION * picks, (model, cname, k, near, picks)
            assert broken >= 1, (model, cname, k)
