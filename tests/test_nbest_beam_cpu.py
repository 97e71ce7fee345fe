"""No GPU: what tests/test_hip_nbest_beam.py rests on.
(a) tests/nbest_oracle.nbest_loop — beam_np.beam_loop restated so that it returns every completed hypothesis — answers what
    beam_loop answers (best entry, score, step-limit answer) and what the reference's own loops recorded (`score`, `ncomplete` of
    tests/golden/beam_*.npz) for every search of beam_small_e3, beam_small_e5, beam_full_b4 and beam_adaptive_small.
(b) The table of the GPU test (nbest_oracle.FIXTURE / SHIFTS / BEAMS / MODELS, six images: 162 searches), printed and pinned: what
    it contains, and that every two neighbouring n-best scores of a search are further apart than beam_parity.MARGIN_MIN — the
    GPU test compares token lists in order, never loosely.
(c) The four n-best entry points: exported, prototyped, refusing bad arguments before any HIP call."""
import collections
import ctypes as C

import numpy as np
import pytest

import beam_parity
import nbest_oracle as NO
from oracle import beam_np, cases, dcnet_np as DN, editnet_np as EN
from test_adaptive_beam_golden_cpu import AdaptiveBeam, boosted_params


def _same_answer(done, limit, limit_seq, ref):
    seq, score, margin = ref
    if np.isnan(score):
        assert limit and limit_seq == seq
        return
    assert not limit
    best = NO.ranked(done)[0]
    assert best[0] == seq and best[1] == score                         # the FIRST maximum: a stable sort keeps completion order
    assert (NO.min_gap(done) if len(done) > 1 else np.inf) <= margin   # (margin: the gap between the two best)


@pytest.mark.parametrize("name", ["beam_small_e3", "beam_small_e5", "beam_full_b4"])
def test_restated_loop_vs_beam_loop_and_the_reference_goldens(name):
    d = cases.build_beam(name)
    g = beam_parity.load(name)
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
            for model in NO.MODELS:
                done, limit, limit_seq = NO.search(model, Pe, Pd, *one, start, end, k)
                _same_answer(done, limit, limit_seq, refs[model]())
                pre = "k%d.%s." % (k, model)
                assert limit == bool(g[pre + "infinite"][b]), (name, k, model, b)
                assert len(done) == int(g[pre + "ncomplete"][b]), (name, k, model, b, len(done))
                if not limit:
                    assert abs(NO.ranked(done)[0][1] - float(g[pre + "score"][b])) < beam_parity.SCORE_TOL, (name, k, model, b)
                n += 1
    assert n == len(d["beams"]) * B * 3


def test_restated_loop_vs_the_adaptive_golden():
    d = cases.build_editnet("editnet_adaptive_small")
    g = beam_parity.load("beam_adaptive_small")
    c, wm = d["case"], d["wm"]
    V = c["V"]
    comb = NO.COMBINE["single"]
    for boost in g["boosts"]:
        P = boosted_params(d["sd"], V, float(boost))
        pre0 = "adaptive_e%d" % int(round(float(boost) * 10))
        for k in (int(x) for x in g["beams"]):
            for b in range(c["B"]):
                mk = lambda: [AdaptiveBeam(P, d["X"][b:b + 1], d["image_mean"][b:b + 1], d["prev"][b:b + 1], d["plen"][b:b + 1], k)]
                done, limit, limit_seq = NO.nbest_loop(mk(), comb, wm["<start>"], wm["<end>"], V, k)
                _same_answer(done, limit, limit_seq, beam_np.beam_loop(mk(), comb, wm["<start>"], wm["<end>"], V, k))
                pre = "k%d.%s." % (k, pre0)
                assert limit == bool(g[pre + "infinite"][b]) and len(done) == int(g[pre + "ncomplete"][b]), (boost, k, b, len(done))
                if not limit:
                    assert abs(NO.ranked(done)[0][1] - float(g[pre + "score"][b])) < beam_parity.SCORE_TOL


def test_the_table_of_the_gpu_test():
    """162 searches.  Pinned: 139 finish, 23 stop at the step limit (none at the shipped bias, 9 with <end> lowered by 1.0, 14
    by 1.5) having completed 0 / 1 / 2 / 3 / 4 hypotheses (6 / 2 / 7 / 4 / 4 searches); 599 completions in all, the last one at
    pick 46; 129 searches complete several hypotheses in one pick; the first completion comes at pick 1 in 151 searches and
    only at pick 3, 4, 9, 10, 10 in five.  The smallest gap between neighbouring n-best scores is 0.0038 (<end> lowered by 1.5,
    k = 5, image 1, DCNet), above MARGIN_MIN = 2e-3: no cell had to be removed."""
    t = NO.table()
    assert len(NO.REMOVED) <= 2 and all(s != 0.0 for s, _, _ in NO.REMOVED)
    assert len(t) == 3 * (len(NO.SHIFTS) * len(NO.BEAMS) * 6 - len(NO.REMOVED))
    for key in sorted(t):
        done, limit, _ = t[key]
        print(key, "limit" if limit else "", [(round(s, 3), pick, len(seq)) for seq, s, pick in done], "min gap %.4f" % NO.min_gap(done))
    gaps = sorted((NO.min_gap(v[0]), key) for key, v in t.items())
    print("smallest gaps", gaps[:4])
    assert all(gap > beam_parity.MARGIN_MIN for gap, _ in gaps), gaps[0]
    assert gaps[0][1] == (-1.5, 5, 1, "dcnet") and 0.0035 < gaps[0][0] < 0.0040
    assert sum(1 for v in t.values() if not v[1]) == 139
    at_limit = collections.Counter(len(v[0]) for v in t.values() if v[1])
    assert dict(at_limit) == {0: 6, 1: 2, 2: 7, 3: 4, 4: 4}
    assert [sum(1 for key, v in t.items() if key[0] == s and v[1]) for s in NO.SHIFTS] == [0, 9, 14]
    assert sum(len(v[0]) for v in t.values()) == 599
    assert max(e[2] for v in t.values() for e in v[0]) == 46
    assert sum(1 for v in t.values() if len({e[2] for e in v[0]}) < len(v[0])) == 129
    first = collections.Counter(min(e[2] for e in v[0]) for v in t.values() if v[0])
    assert dict(first) == {1: 151, 3: 1, 4: 1, 9: 1, 10: 2}
    wm = cases.build_beam(NO.FIXTURE)["wm"]
    for (shift, k, b, model), (done, limit, _) in t.items():           # at most k completions; all k when the search finished
        assert all(seq[0] == wm["<start>"] and seq[-1] == wm["<end>"] for seq, _, _ in done)
        assert len(done) <= k and (limit or len(done) == k)


# ---- (c) ABI
@pytest.fixture(scope="module")
def lib():
    from show_edit_tell_amd import _lib
    return _lib.load()


def test_entry_points_are_exported_and_prototyped(lib):
    from show_edit_tell_amd import _lib
    for name, old in (("set_beam_pick_nbest_f32", "set_beam_pick_f32"), ("set_editnet_beam_persistent_nbest", "set_editnet_beam_persistent"),
                      ("set_dcnet_beam_persistent_nbest", "set_dcnet_beam_persistent"),
                      ("set_ensemble_beam_persistent_nbest", "set_ensemble_beam_persistent")):
        assert name in _lib.PROTOTYPES and name not in _lib.MISSING
        extra = 4 if name == "set_beam_pick_nbest_f32" else 1
        assert len(getattr(lib, name).argtypes) == len(getattr(lib, old).argtypes) + extra


def test_refusals_are_those_of_the_entries_without_n_best(lib):
    """SET_ERR_ARG = 1 for a NULL n-best array and for what the old entry refuses; SET_ERR_UNSUPPORTED = 2 as before (no token
    table, k > BEAM_KMAX): all answered before any HIP call, no device needed."""
    from show_edit_tell_amd._lib import DcnetDims, DcnetWeights, EditNetDims, EditNetWeights
    one = C.c_void_p(16)                      # (never dereferenced: the checks come first)
    de = EditNetDims(B=3, T=18, R=36, F=2048, D=1024, A=512, V=10000, maxT=51, adaptive=0)
    dd = DcnetDims(B=3, T=18, D=1024, A=512, C=512, E=1024, V=10000, maxT=51)
    we, wd = EditNetWeights(), DcnetWeights()
    e = lambda hs=one, picks=51, start=0: lib.set_editnet_beam_persistent_nbest(C.byref(we), C.byref(de), one, None, one, one, start, 1, picks,
                                                                                one, one, one, one, one, one, 0, None, hs)
    dn = lambda hs=one, picks=51, start=0: lib.set_dcnet_beam_persistent_nbest(C.byref(wd), C.byref(dd), one, one, start, 1, picks, one, one,
                                                                               one, one, one, one, 0, None, hs)
    en = lambda hs=one, picks=51, start=0: lib.set_ensemble_beam_persistent_nbest(C.byref(we), C.byref(de), C.byref(wd), C.byref(dd), one, one,
                                                                                  one, start, 1, picks, one, one, one, one, one, one, 0, one,
                                                                                  0, one, 0, None, hs)
    for f in (e, dn, en):
        assert f(hs=None) == 1 and f(picks=0) == 1 and f(start=10000) == 1
        assert f() == 2                       # no token table
    pick = lambda k=3, ds=one, nd=one, cur=1: lib.set_beam_pick_nbest_f32(one, None, 100, 2, k, 100, 99, cur, 8, one, one, one, one, one, one,
                                                                          one, one, one, ds, one, one, nd, None)
    assert pick(ds=None) == 1 and pick(nd=None) == 1 and pick(cur=0) == 1 and pick(cur=8) == 1
    assert pick(k=9) == 2


def test_n_best_is_validated_before_anything_else():
    from show_edit_tell_amd import evaluate
    for bad in (0, 4, -1, 1.5):
        with pytest.raises(ValueError):
            evaluate._check_n_best(bad, 3)
    assert evaluate._check_n_best(None, 3) is None and evaluate._check_n_best(3, 3) == 3 and evaluate._check_n_best(1, 3) == 1
    for f in (evaluate.beam_search_dcnet, evaluate.beam_search_dcnet_batched):
        with pytest.raises(ValueError):
            f(None, None, None, {}, 3, n_best=4)
    assert evaluate._n_best_sorted([([1], -2.0), ([2], -1.0), ([3], -2.0), ([4], -1.0)], 3) == [([2], -1.0), ([4], -1.0), ([1], -2.0)]
