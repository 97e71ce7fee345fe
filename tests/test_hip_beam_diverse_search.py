"""GPU: evaluate.beam_search_diverse / beam_search_diverse_ensemble on beam_small_e5's models with <end> lowered (the models, shift
and images of tests/beam_constrained_fixtures.py's search fixture; (k, G) = (4, 2) and (6, 3), max_steps 20).  A host-driven replay
(the same _FusedModel steps, the logits copied to the host, the float64 oracle's pick, index_select for the state) agrees with the
device search wherever the oracle's margin is >= GAP, by the method of tests/test_hip_beam_constrained_search.py; group 0 is the
plain search of g slots; a very large penalty makes the groups' first words differ; no result violates the constraints;
return_all lists every completion with its group."""
import numpy as np
import pytest
import torch

import beam_constrained_fixtures as F
import beam_diverse_fixtures as D
import beam_diverse_oracle as DO
import nbest_oracle as NO
from test_beam_diverse_cpu import near_ties
from test_hip_beam_constrained_search import _cons, _entries, _setup

pytestmark = pytest.mark.gpu


def _diverse(model, k, G, penalty, c, **kw):
    from show_edit_tell_amd import evaluate as ev
    wm, xe, dae, X, prev, plen = _setup()
    kw = dict(beam_size=k, groups=G, diversity_penalty=penalty, max_steps=D.SEARCH_MAX_STEPS, constraints=_cons(c), **kw)
    if model == "editnet":
        return ev.beam_search_diverse(xe, X, prev, plen, wm, **kw)
    if model == "dcnet":
        return ev.beam_search_diverse(dae, prev, plen, wm, **kw)
    return ev.beam_search_diverse_ensemble(xe, dae, X, prev, plen, wm, **kw)


def _replay(model, k, G, penalty, c):
    """the search driven from the host on the oracle's pick -> DO.search's (answers, completed, steps)"""
    from show_edit_tell_amd import evaluate as ev
    wm, xe, dae, X, prev, plen = _setup()
    pl = plen.reshape(-1).long().contiguous()
    ms = []
    if model in ("editnet", "ensemble"):
        ms.append(ev._FusedModel(xe, (X.float().contiguous(), None, prev, pl), (X.float().contiguous(),), k, D.SEARCH_MAX_STEPS))
    if model in ("dcnet", "ensemble"):
        ms.append(ev._FusedModel(dae, (prev, pl), (), k, D.SEARCH_MAX_STEPS))
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
        return DO.search(step, reindex, F.SEARCH_NI, k, V, int(wm["<start>"]), int(wm["<end>"]), c, D.SEARCH_MAX_STEPS, G, penalty)


def _close(a, b, n):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= F.TOL * n


@pytest.mark.parametrize("model", NO.MODELS)
@pytest.mark.parametrize("k,G", D.SEARCH_SHAPES)
def test_searches_against_the_host_driven_replay(model, k, G):
    """neutral constraints and "all", the fixture's penalty and the very large one: the G answers and the return_all list against
    the replay — the same tokens and groups, scores within TOL x tokens — for every image whose counted picks all keep the oracle's
    key margin >= GAP; an image with a closer pick may differ, and such picks stay within NEAR_TIE_FRACTION of all picks.  Every
    result obeys the constraints; the list is sorted by score and holds every group's answer; with the very large penalty the
    groups' first words differ pairwise; group 0 returns what the plain batched search of g slots returns."""
    wm, xe, dae, X, prev, plen = _setup()
    start, end = int(wm["<start>"]), int(wm["<end>"])
    g = k // G
    plain_f = _entries(model)[1]
    picks = near = matched = 0
    for cname, c in sorted(D.search_constraints().items()):
        plain = plain_f(X, prev, plen, g, return_scores=True, constraints=_cons(c))
        for penalty in (D.SEARCH_PENALTY, D.SEARCH_BIG_PENALTY):
            out, every = _diverse(model, k, G, penalty, c, return_all=True)
            ans, done, steps = _replay(model, k, G, penalty, c)
            for i in range(F.SEARCH_NI):
                p, n = near_ties(steps, i)
                picks, near = picks + p, near + n
                print(model, (k, G), cname, penalty, "image", i, out[i], "near ties", n, "of", p)
                assert len(out[i]) == G
                for gi, (seq, sc) in enumerate(out[i]):
                    assert not F.violates(seq, c, end), (cname, i, gi, seq)
                    if not np.isnan(sc):
                        assert (seq, sc, gi) in every[i], (cname, i, gi)
                assert all(a[1] >= b[1] for a, b in zip(every[i], every[i][1:])), (cname, i, every[i])
                assert all(s[-1] == end and 0 <= gi < G and not F.violates(s, c, end) for s, _, gi in every[i]), (cname, i)
                if penalty == D.SEARCH_BIG_PENALTY:
                    first = [seq[1] for seq, _ in out[i] if len(seq) > 1 and seq[1] != end]
                    assert len(set(first)) == len(first), (cname, i, out[i])
                if n:
                    continue
                assert [s for s, _ in out[i]] == [s for s, _ in ans[i]], (cname, i, out[i], ans[i])
                assert all(_close(a[1], b[1], len(a[0])) for a, b in zip(out[i], ans[i])), (cname, i, out[i], ans[i])
                assert [(s, gi) for s, _, gi in every[i]] == [(s, gi) for s, _, gi in done[i]], (cname, i, every[i], done[i])
                assert all(_close(a[1], b[1], len(a[0])) for a, b in zip(every[i], done[i])), (cname, i)
                # group 0 is never penalised: the plain search of g slots (another GEMM tile height: compared where no pick is close)
                if not np.isnan(plain[1][i]) and not np.isnan(out[i][0][1]):
                    assert out[i][0][0] == plain[0][i] and _close(out[i][0][1], plain[1][i], len(plain[0][i])), (cname, i, out[i][0], plain[0][i])
                    matched += 1
    assert near <= F.NEAR_TIE_FRACTION * picks, (near, picks)
    assert matched > 0
