"""No GPU: what tests/test_hip_ensemble_beam.py rests on.
(a) The numpy oracle's outcome table (oracle/beam_np.beam_ensemble) for the 36 searches of the GPU test — beam_full_b4 with
    fc.bias[<end>] of both models changed from 4.0 to 2.2 / 2.7 / 2.8, k = 2 / 3 / 4, four images — so that the floors the GPU
    test asks for cannot silently become vacuous if a fixture changes.
(b) A numpy restatement of the launch's two-round slice pick (csrc/decode_persistent_ensemble.hip P1 - P3) against the flat
    stable top-k of log((softmax_e + softmax_d) / 2) + score.
(c) The C ABI and the Python routing of set_ensemble_beam_persistent / evaluate.beam_search_ensemble."""
import ctypes as C

import numpy as np
import pytest

from oracle import beam_np, cases, dcnet_np as DN, editnet_np as EN

BOOSTS, BEAMS = (2.2, 2.7, 2.8), (2, 3, 4)


def _boosted(d, boost):
    end = d["wm"]["<end>"]
    out = []
    for key in ("sd_e", "sd_d"):
        sd = {k: v.copy() for k, v in d[key].items()}
        sd["fc.bias"][end] = sd["fc.bias"][end] - np.float32(4.0) + np.float32(boost)
        out.append(sd)
    return out


@pytest.fixture(scope="module")
def case():
    return cases.build_beam("beam_full_b4")


def test_oracle_outcome_table_of_the_36_searches(case):
    d = case
    wm, B = d["wm"], d["case"]["B"]
    start, end = wm["<start>"], wm["<end>"]
    table, margins = {}, []
    for boost in BOOSTS:
        sd_e, sd_d = _boosted(d, boost)
        Pe, Pd = EN.cast_params(sd_e), DN.cast_params(sd_d)
        for k in BEAMS:
            for b in range(B):
                seq, score, margin = beam_np.beam_ensemble(Pe, Pd, d["X"][b:b + 1], d["prev"][b:b + 1], d["plen"][b:b + 1], start, end, k)
                table[(boost, k, b)] = None if np.isnan(score) else len(seq)
                if not np.isnan(score):
                    margins.append((float(margin), boost, k, b))
    print(table)
    finished = [v for v in table.values() if v is not None]
    assert len(table) == 36
    assert len(finished) == 23 and sum(v is None for v in table.values()) == 13
    assert sum(1 for v in finished if v >= 5) == 6 and sorted(v for v in finished if v >= 5)[0] >= 6 and max(finished) == 14
    assert all(table[(boost, k, 1)] is None for boost in BOOSTS for k in BEAMS)            # image 1: the step limit at every boost
    assert [table[(2.7, k, 2)] for k in BEAMS] == [6, 14, 13]
    assert [table[(2.8, k, 2)] for k in BEAMS] == [6, 9, 9]
    assert all(table[(2.2, k, 2)] is None for k in BEAMS)
    worst = min(margins)
    print("smallest margin", worst)
    assert worst[0] >= 4.98 and worst[1:] == (2.7, 4, 2), worst


# ---- (b) the slice pick
def _slice_pick(le, ld, score, k, V, G=256):
    """Float32 restatement of the kernel's joint pick.  le, ld (k, V) logits of the two models, score (k) running scores (-inf =
    dead slot).  Round 1: per live row, model and slice (max, sum exp), combined over the G slices in slice order.  Round 2: per
    live row and word lp = log((exp(le - lse_e) + exp(ld - lse_d)) * 0.5), candidate = score + lp, the slice's 4 best by (value
    descending, flat index ascending).  Merge: the k best of all candidates by the same order."""
    f = np.float32
    rpw = (V + G - 1) // G
    cands = []
    for j in range(k):
        if score[j] == -np.inf:
            continue
        lse = []
        for x in (le[j], ld[j]):
            pm, ps = [], []
            for s in range(G):
                sl = x[s * rpw:min(V, (s + 1) * rpw)].astype(f)
                if sl.size == 0:
                    pm.append(f(-np.inf)); ps.append(f(0))
                    continue
                m = sl.max()
                pm.append(m); ps.append(np.exp(sl - m, dtype=f).sum(dtype=f))
            m = max(pm)
            tot = f(0)
            for a, b in zip(pm, ps):
                if a != -np.inf:
                    tot = f(tot + b * np.exp(f(a - m), dtype=f))
            lse.append(f(m + np.log(tot, dtype=f)))
        lp = np.log((np.exp(le[j].astype(f) - lse[0], dtype=f) + np.exp(ld[j].astype(f) - lse[1], dtype=f)) * f(0.5), dtype=f)
        val = (f(score[j]) + lp).astype(f)
        for s in range(G):
            lo, hi = s * rpw, min(V, (s + 1) * rpw)
            if lo >= hi:
                continue
            idx = sorted(range(lo, hi), key=lambda v: (-val[v], v))[:4]
            cands += [(-float(val[v]), j * V + v) for v in idx]
    cands.sort()
    return [(flat // V, flat % V, -nv) for nv, flat in cands[:k]]


def _flat_pick(le, ld, score, k, V):
    comb = np.log((EN._softmax(le, 1) + EN._softmax(ld, 1)) / 2)
    flat = (score[:, None].astype(np.float32) + comb).reshape(-1)
    order = np.argsort(-flat, kind="stable")[:k]
    return [(int(o // V), int(o % V), float(flat[o])) for o in order]


def _recorded_picks(d, boost, b, k, picks):
    """(le, ld, score) of the oracle's search of image b at the given pick numbers (1-based), beam_np.beam_loop's bookkeeping."""
    wm = d["wm"]
    start, end = wm["<start>"], wm["<end>"]
    sd_e, sd_d = _boosted(d, boost)
    Pe, Pd = EN.cast_params(sd_e), DN.cast_params(sd_d)
    V = Pe["fc.weight"].shape[0]
    X1, prev1, plen1 = d["X"][b:b + 1], d["prev"][b:b + 1], d["plen"][b:b + 1]
    states = [beam_np.EditNetBeam(Pe, X1, prev1, plen1, k), beam_np.DcnetBeam(Pd, prev1, plen1, k)]
    words = np.full((k,), start, np.int64)
    top = np.zeros((k,), np.float32)
    out, step = [], 1
    while k > 0 and step <= max(picks):
        ls = [s.step(words) for s in states]
        score = top.copy()
        if step == 1:
            score[1:] = -np.inf                               # all rows are identical: only row 0 counts
        if step in picks:
            out.append((ls[0].copy(), ls[1].copy(), score.copy(), len(words)))
        win = _flat_pick(ls[0], ls[1], score, len(words), V)
        inc = [i for i, (_, w, _) in enumerate(win) if w != end]
        k = len(inc)
        if k == 0:
            break
        parent = np.array([win[i][0] for i in inc])
        for s in states:
            s.reindex(parent)
        top = np.array([win[i][2] for i in inc], np.float32)
        words = np.array([win[i][1] for i in inc], np.int64)
        step += 1
    return out, V


@pytest.mark.parametrize("k", BEAMS)
def test_two_round_slice_pick_equals_the_flat_top_k(case, k):
    """The logits of picks 1, 2, 3 and 5 of the long search (boost 2.7, image 2), as they are, with a dead slot, and with an
    exact tie across two slices: the same (parent, word) winners in the same order, scores within 1e-5."""
    rec, V = _recorded_picks(case, 2.7, 2, k, (1, 2, 3, 5))
    assert len(rec) >= 3
    rpw = (V + 255) // 256
    checked = ties = 0
    for le, ld, score, kk in rec:
        variants = [(le, ld, score)]
        if kk > 1 and np.isfinite(score).sum() > 1:
            dead = score.copy(); dead[kk - 1] = -np.inf                          # a dead slot
            variants.append((le, ld, dead))
        j0, v0, _ = _flat_pick(le, ld, score, kk, V)[0]
        v1 = (v0 + 3 * rpw + 1) % V                                             # a word of another slice gets the winner's logits
        assert v1 // rpw != v0 // rpw
        le2, ld2 = le.copy(), ld.copy()
        le2[j0, v1], ld2[j0, v1] = le2[j0, v0], ld2[j0, v0]
        variants.append((le2, ld2, score))
        for n, (a, b_, s) in enumerate(variants):
            want, got = _flat_pick(a, b_, s, kk, V), _slice_pick(a, b_, s, kk, V)
            assert [(p, w) for p, w, _ in got] == [(p, w) for p, w, _ in want], (k, n, got, want)
            assert all(abs(x[2] - y[2]) < 1e-5 for x, y in zip(got, want)), (k, n, got, want)
            if a is le2:                                                         # the tie: equal values, ascending flat index
                at = [i for i, (p, w, _) in enumerate(got) if p == j0 and w in (v0, v1)]
                if len(at) == 2:
                    i0, i1 = at
                    assert i1 == i0 + 1 and got[i0][2] == got[i1][2] and [got[i0][1], got[i1][1]] == sorted((v0, v1)), got
                    ties += 1
            checked += 1
    assert checked >= 6 and ties >= 1


# ---- (c) ABI and routing
@pytest.fixture(scope="module")
def lib():
    from show_edit_tell_amd import _lib
    return _lib.load()


def test_entry_points_are_exported_and_prototyped(lib):
    from show_edit_tell_amd import _lib
    for name, nargs in (("set_ensemble_beam_persistent", 22), ("set_ensemble_beam_xbuf_bytes", 2)):
        assert name in _lib.PROTOTYPES and name not in _lib.MISSING
        assert len(getattr(lib, name).argtypes) == nargs


def test_bad_arguments_and_mismatched_models_are_refused_before_any_hip_call(lib):
    """SET_ERR_ARG = 1: null pointers, max_picks < 1, a start token outside the vocabulary.  SET_ERR_UNSUPPORTED = 2: rows, T or
    vocabulary size differ between the models, an adaptive decoder, k > 4, no token table.  No device is needed."""
    from show_edit_tell_amd._lib import DcnetDims, DcnetWeights, EditNetDims, EditNetWeights
    E = lambda **kw: EditNetDims(**dict(dict(B=3, T=18, R=36, F=2048, D=1024, A=512, V=10000, maxT=51, adaptive=0), **kw))
    Dd = lambda **kw: DcnetDims(**dict(dict(B=3, T=18, D=1024, A=512, C=512, E=1024, V=10000, maxT=51), **kw))
    we, wd = EditNetWeights(), DcnetWeights()
    one = C.c_void_p(16)                      # (never dereferenced: the checks come first)

    def call(de=None, dd=None, X=one, start=0, picks=51, result=one, xbuf=one):
        de, dd = de or E(), dd or Dd()
        return lib.set_ensemble_beam_persistent(C.byref(we), C.byref(de), C.byref(wd), C.byref(dd), X, one, one, start, 1, picks, one, one,
                                                one, one, result, one, 0, one, 0, xbuf, 0, None)

    assert lib.set_ensemble_beam_persistent(None, None, None, None, None, None, None, 0, 1, 51, None, None, None, None, None, None, 0,
                                            None, 0, None, 0, None) == 1
    assert call(X=None) == 1 and call(result=None) == 1 and call(xbuf=None) == 1
    assert call(picks=0) == 1
    assert call(start=10000) == 1 and call(start=-1) == 1
    assert call(dd=Dd(B=4)) == 2
    assert call(dd=Dd(T=20)) == 2
    assert call(dd=Dd(V=9936)) == 2 and call(de=E(V=9936)) == 2
    assert call(de=E(adaptive=1)) == 2
    assert call(de=E(B=5), dd=Dd(B=5)) == 2
    assert call() == 2                        # no token table
    assert lib.set_ensemble_beam_xbuf_bytes(C.byref(E()), C.byref(Dd())) == 128 + 8 * 3 * (6 * 1024 + 1024 + 32 + 64 + 512 + 256 * 16)
    assert lib.set_ensemble_beam_xbuf_bytes(C.byref(E()), C.byref(Dd(B=4))) == 0
    assert lib.set_ensemble_beam_xbuf_bytes(C.byref(E(adaptive=1)), C.byref(Dd())) == 0


def test_workspace_sizes_did_not_change(lib):
    """The launch's exchange region is a buffer of its own: the sizes the two workspace queries report are those of the
    single-model launches (pinned in tests/test_dcnet_beam_cpu.py for DCNet; the same per-row law for EditNet)."""
    from show_edit_tell_amd._lib import EditNetDims
    n = {B: lib.set_editnet_workspace_bytes(C.byref(EditNetDims(B=B, T=18, R=36, F=2048, D=1024, A=512, V=10000, maxT=19, adaptive=0)))
         for B in (3, 4, 5, 6, 7)}
    per_row, slack = 256 * 12 * 8, 64 * 256
    assert abs((n[7] - n[6]) - (n[6] - n[5])) <= slack
    assert abs((n[4] - n[3]) - (n[6] - n[5]) - per_row) <= slack
    assert abs((n[5] - n[4]) - (n[6] - n[5]) + 4 * per_row) <= slack


def test_beam_search_ensemble_tries_the_persistent_launch_first(monkeypatch):
    from show_edit_tell_amd import evaluate
    calls = []

    def persistent(dec, dae, X, prev, plen, wm, k, *a, **kw):
        calls.append(("persistent", k))
        return persistent.answer

    def batched(dec, dae, X, prev, plen, wm, k=3, *a, **kw):
        calls.append(("batched", k))
        assert kw.get("return_scores")
        return [[7, 8, 9]], [-1.5]

    monkeypatch.setattr(evaluate, "_beam_search_ensemble_persistent", persistent)
    monkeypatch.setattr(evaluate, "beam_search_ensemble_batched", batched)
    persistent.answer = ([1, 2, 3], -0.25)
    assert evaluate.beam_search_ensemble(None, None, None, None, None, {}, 3) == ([1, 2, 3], -0.25)
    assert calls == [("persistent", 3)]
    del calls[:]
    persistent.answer = None                  # SET_ERR_UNSUPPORTED: the batched per-step search answers
    assert evaluate.beam_search_ensemble(None, None, None, None, None, {}, 5) == ([7, 8, 9], -1.5)
    assert calls == [("persistent", 5), ("batched", 5)]


def test_host_side_refusals_need_no_device():
    """k outside 1 .. 4, more than one image, vocabularies of different size, an adaptive decoder: None before the library is
    touched."""
    import torch
    from show_edit_tell_amd import evaluate

    class M:
        vocab_size = 100
        _adaptive = 0

    class M2(M):
        vocab_size = 90

    class MA(M):
        _adaptive = 1

    X, prev, plen = torch.zeros(1, 36, 8), torch.zeros(1, 18, dtype=torch.long), torch.ones(1, 1, dtype=torch.long)
    f = evaluate._beam_search_ensemble_persistent
    assert f(M(), M(), X, prev, plen, {}, 0) is None and f(M(), M(), X, prev, plen, {}, 5) is None
    assert f(M(), M(), X.expand(2, -1, -1), prev.expand(2, -1), plen.expand(2, -1), {}, 3) is None
    assert f(M(), M2(), X, prev, plen, {}, 3) is None
    assert f(MA(), M(), X, prev, plen, {}, 3) is None
