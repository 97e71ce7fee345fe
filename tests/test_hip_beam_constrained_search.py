"""GPU: the eight evaluate.beam_search_* entries with `constraints=` on beam_small_e5's models with <end> lowered
(tests/beam_constrained_fixtures.py: three images, k = 3 and 5, max_steps 20).  Neutral constraints change nothing; a host-driven
replay (the same _FusedModel steps, the logits copied to the host, the float64 oracle's pick, index_select for the state) agrees
with the device search wherever the oracle's margin is >= GAP; the results obey the constraints that the unconstrained results
break; return_trace traces the constrained tokens."""
import numpy as np
import pytest
import torch

import beam_constrained_fixtures as F
import beam_constrained_oracle as BO
import nbest_oracle as NO
from hip_adapter import adaptive_module, load_numpy_state, to_dev
from oracle import cases

pytestmark = pytest.mark.gpu
_CACHE = {}


def _setup():
    """(word map, EditNet, DCNet, inputs of the fixture's three images): built once"""
    if "m" not in _CACHE:
        from show_edit_tell_amd import dcnet, editnet
        d = cases.build_beam(F.SEARCH_FIXTURE)
        c, dc, wm = d["case"], d["dcase"], d["wm"]
        sd_e, sd_d = NO.shifted(d, F.SEARCH_SHIFT)
        xe = load_numpy_state(editnet.DecoderC(wm, c["D"], c["D"], c["D"], c["A"], c["F"]), sd_e)
        dae = load_numpy_state(dcnet.DAE(wm, None, dc["D"], dc["A"], dc["C"], dc["E"]), sd_d)
        idx = list(F.SEARCH_IMAGES)
        _CACHE["m"] = (wm, xe, dae, to_dev(d["X"][idx]), to_dev(d["prev"][idx]), to_dev(d["plen"][idx]))
    return _CACHE["m"]


def _entries(model):
    """(per-image entry, batched entry) of one model as functions of (X, prev, plen, k, **kw)"""
    from show_edit_tell_amd import evaluate as ev
    wm, xe, dae = _setup()[:3]
    if model == "editnet":
        return (lambda X, p, l, k, **kw: ev.beam_search_editnet(xe, X, p, l, wm, k, **kw),
                lambda X, p, l, k, **kw: ev.beam_search_editnet_batched(xe, X, p, l, wm, k, max_steps=F.SEARCH_MAX_STEPS, **kw))
    if model == "dcnet":
        return (lambda X, p, l, k, **kw: ev.beam_search_dcnet(dae, p, l, wm, k, **kw),
                lambda X, p, l, k, **kw: ev.beam_search_dcnet_batched(dae, p, l, wm, k, max_steps=F.SEARCH_MAX_STEPS, **kw))
    return (lambda X, p, l, k, **kw: ev.beam_search_ensemble(xe, dae, X, p, l, wm, k, **kw),
            lambda X, p, l, k, **kw: ev.beam_search_ensemble_batched(xe, dae, X, p, l, wm, k, max_steps=F.SEARCH_MAX_STEPS, **kw))


def _cons(c):
    from show_edit_tell_amd import evaluate as ev
    return ev.BeamConstraints(no_repeat_ngram=c.no_repeat_ngram, min_length=c.min_len, length_penalty=c.length_alpha,
                              banned_words=c.banned)


def _same(a, b):
    """results equal, NaN scores equal to NaN"""
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b or (isinstance(a, float) and isinstance(b, float) and np.isnan(a) and np.isnan(b))


def test_none_and_neutral_constraints_change_nothing():
    """all eight entries, with scores and the n-best list: `constraints=None` and BeamConstraints() return exactly what the call
    without the keyword returns"""
    from show_edit_tell_amd import evaluate as ev
    wm, xe, dae, X, prev, plen = _setup()
    calls = []
    for model in NO.MODELS:
        one_f, many_f = _entries(model)
        calls.append(lambda kw, f=one_f: f(X[1:2], prev[1:2], plen[1:2], 3, n_best=3, **kw))
        calls.append(lambda kw, f=many_f: f(X, prev, plen, 3, return_scores=True, n_best=2, **kw))
    da, dec = adaptive_module("editnet_adaptive_small")
    Xa, mean, pa, la = to_dev(da["X"]), to_dev(da["image_mean"]), to_dev(da["prev"]), to_dev(da["plen"])
    calls.append(lambda kw: ev.beam_search_adaptive(dec, Xa[:1], mean[:1], pa[:1], la[:1], da["wm"], 3, n_best=3, **kw))
    calls.append(lambda kw: ev.beam_search_adaptive_batched(dec, Xa, mean, pa, la, da["wm"], 3, max_steps=F.SEARCH_MAX_STEPS,
                                                           return_scores=True, n_best=2, **kw))
    assert len(calls) == 8
    for n, call in enumerate(calls):
        call({})                                                         # (the token tables are built on the first calls)
        call({})
        base = call({})
        assert _same(call(dict(constraints=None)), base), n
        assert _same(call(dict(constraints=ev.BeamConstraints())), base), n


def _replay(model, k, c):
    """the search driven from the host on the oracle's pick -> BO.search's (answers, nbest, steps)"""
    from show_edit_tell_amd import evaluate as ev
    wm, xe, dae, X, prev, plen = _setup()
    pl = plen.reshape(-1).long().contiguous()
    ms = []
    if model in ("editnet", "ensemble"):
        ms.append(ev._FusedModel(xe, (X.float().contiguous(), None, prev, pl), (X.float().contiguous(),), k, F.SEARCH_MAX_STEPS))
    if model in ("dcnet", "ensemble"):
        ms.append(ev._FusedModel(dae, (prev, pl), (), k, F.SEARCH_MAX_STEPS))
    V, dev = xe.vocab_size, X.device
    bufs = [torch.empty(F.SEARCH_NI * k, V, device=dev) for _ in ms]

    def step(words):
        w = torch.from_numpy(words).to(dev)
        for m, lg in zip(ms, bufs):
            m.step(w, lg)
        return [lg.cpu().numpy() for lg in bufs]

    def reindex(rows):
        r = torch.from_numpy(rows.astype(np.int64)).to(dev)
        for m in ms:
            for s in m.states:
                s.copy_(s.index_select(0, r))
    with torch.no_grad():
        return BO.search(step, reindex, F.SEARCH_NI, k, V, int(wm["<start>"]), int(wm["<end>"]), c, F.SEARCH_MAX_STEPS)


@pytest.mark.parametrize("model", NO.MODELS)
@pytest.mark.parametrize("k", F.SEARCH_BEAMS)
def test_searches_against_the_host_driven_replay_and_the_constraints(model, k):
    """every constraint set of the fixture: the batched search (scores, n_best = k) against the replay — the same tokens, n-best
    lists and scores within TOL for every image whose picks all keep the oracle's margin >= GAP; an image with a closer pick may
    differ, and such picks stay within NEAR_TIE_FRACTION of all picks.  (A score is a sum of one log-probability per token, each
    within TOL of the oracle's on the same float32 logits: TOL x tokens.)  Primary results and every n-best entry repeat no n-gram,
    hold no banned word and are at least min_length long; the lists are sorted by r.  Precondition: some unconstrained result
    breaks the rule.  The per-image entry obeys the same rules."""
    wm, xe, dae, X, prev, plen = _setup()
    end = int(wm["<end>"])
    one_f, many_f = _entries(model)
    many_f(X, prev, plen, k)                                             # (token tables)
    free = many_f(X, prev, plen, k, n_best=k)
    picks = near = 0
    for cname, c in sorted(F.search_constraints().items()):
        assert any(F.violates(s, c, end) for s in free[0]) or any(F.violates(s, c, end) for nb in free[1] for s, _ in nb), cname
        seqs, scores, lists = many_f(X, prev, plen, k, return_scores=True, n_best=k, constraints=_cons(c))
        ans, nbest, steps = _replay(model, k, c)
        for i in range(F.SEARCH_NI):
            gaps = []
            for info in steps:
                if info[i]:
                    v = [x for x, _ in info[i]["top"]]
                    gaps += [p - q for p, q in zip(v, v[1:])][:info[i]["counted"]]
            picks += len(gaps)
            close = sum(1 for g in gaps if g < F.GAP)
            near += close
            print(model, k, cname, "image", i, seqs[i], scores[i], "smallest margin %.2e" % min(gaps, default=np.inf))
            for s in [seqs[i]] + [s for s, _ in lists[i]]:
                assert not F.violates(s, c, end), (cname, i, s)
            assert all(s[-1] == end and len(s) - 2 >= c.min_len for s, _ in lists[i]), (cname, i, lists[i])
            assert all(a[1] >= b[1] for a, b in zip(lists[i], lists[i][1:])), (cname, i, lists[i])
            if close:
                continue
            assert seqs[i] == ans[i][0], (cname, i, seqs[i], ans[i])
            assert (np.isnan(scores[i]) and np.isnan(ans[i][1])) or abs(scores[i] - ans[i][1]) <= F.TOL * len(seqs[i]), (cname, i)
            assert [s for s, _ in lists[i]] == [s for s, _ in nbest[i]], (cname, i, lists[i], nbest[i])
            assert all(abs(a[1] - b[1]) <= F.TOL * len(a[0]) for a, b in zip(lists[i], nbest[i])), (cname, i)
        # the per-image entry (the NI = 1 case: other GEMM tiles, so compared by the rules, not token by token)
        res = one_f(X[1:2], prev[1:2], plen[1:2], k, n_best=k, constraints=_cons(c))
        assert len(res) == 3 and not any(F.violates(s, c, end) for s in [res[0]] + [s for s, _ in res[2]]), (cname, res)
        assert all(a[1] >= b[1] for a, b in zip(res[2], res[2][1:])) and (np.isnan(res[1]) or (res[0], res[1]) == res[2][0]), (cname, res)
    assert near <= F.NEAR_TIE_FRACTION * picks, (near, picks)


def test_return_trace_traces_the_constrained_tokens():
    from show_edit_tell_amd import evaluate as ev
    wm, xe, dae, X, prev, plen = _setup()
    c = _cons(F.search_constraints()["all"])
    seqs, tr = ev.beam_search_editnet_batched(xe, X, prev, plen, wm, 3, max_steps=F.SEARCH_MAX_STEPS, return_trace=True, constraints=c)
    assert seqs == ev.beam_search_editnet_batched(xe, X, prev, plen, wm, 3, max_steps=F.SEARCH_MAX_STEPS, constraints=c)
    for i, s in enumerate(seqs):
        assert tr.tokens[i, :len(s)].tolist() == s
    tok, sc, tr1 = ev.beam_search_editnet(xe, X[1:2], prev[1:2], plen[1:2], wm, 3, return_trace=True, constraints=c)
    assert tr1.tokens[0, :len(tok)].tolist() == tok and not F.violates(tok, F.search_constraints()["all"], int(wm["<end>"]))
