"""GPU: the word edit distance on the device (csrc/editdist_device.hip ed_score_k, editdist.DeviceEditDistance) against the
independent restatement tests/edit_oracle.py: statistics and scores on the CPU grid and at the edges of the 64-bit recurrence
under both sentence conventions, the id limit, what the host cannot check and the memory contract, launch independence, pair
scores and the consensus rerank, and the records shared with BLEU.

Tolerances.  The statistics are integers: equality.  A score is ONE correctly rounded double division of two integers below 65,
on the device as in Python, so the expected difference is 0; 1e-12 absolute, the project's bound for these double scores, is
asserted.  The corpus similarity is a mean of up to 250 such values in [0, 1] summed in another order: a few 1e-16."""
import json
import os

import numpy as np
import pytest
import torch

import edit_oracle
from hip_adapter import to_dev

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-12
SENT_I, SENT_F = -777, -12345.678
MEASURED = {}


def _report(name, value):
    """the measured maxima, printed and (SET_EDIT_ERRORS_OUT=file) collected for profiles/edit_device_errors.json"""
    MEASURED[name] = max(float(value), MEASURED.get(name, 0.0))
    print("measured %s = %.3e" % (name, value))
    out = os.environ.get("SET_EDIT_ERRORS_OUT")
    if out:
        prev = {}
        if os.path.exists(out):
            with open(out) as f:
                prev = json.load(f)
        prev.update(MEASURED)
        with open(out, "w") as f:
            json.dump(prev, f, indent=1, sort_keys=True)


def _build(zero_rule):
    """The grid of tests/test_edit_cpu.py plus the edge cases, every hypothesis with its own reference set.
    zero_rule: the sentences carry the token 0 where the rule can say it — a sentence shorter than 64 ids ends with 0 (an empty
    one becomes [0]), every other one of 64 ids too, the rest are full rows without 0 — and rows are cut after their first 0;
    otherwise rows carry explicit lengths and junk (0s included) behind them, and two sentences hold a 0 in their middle."""
    rng = np.random.default_rng(7 if zero_rule else 8)
    pairs = [(list(h), [list(r) for r in R]) for h, R in edit_oracle.grid() + edit_oracle.edge_cases()]
    if zero_rule:
        def end(s, k):
            if len(s) == 0:
                return [0]
            return s[:-1] + [0] if (len(s) < 64 or k % 2) else s
        pairs = [(end(h, i), [end(r, i + j) if (len(r) and j != 1) else r for j, r in enumerate(R)]) for i, (h, R) in enumerate(pairs)]
        pairs.append(([3, 0], [[3, 4, 0], [3, 0]]))                # as the row [3, 0, 4, 5] reads under the rule
    else:
        pairs.append(([3, 0, 4, 5], [[3, 4, 0], [4, 0], [3, 5, 0]]))           # the 0 is a token like any other
        pairs.append(([0, 0, 7], [[7, 0]]))                        # (references are cut after their first 0 under both rules)
    hyps, sets = [p[0] for p in pairs], [p[1] for p in pairs]
    N, L = len(hyps), 64
    H = np.zeros((N, L), dtype=np.int64)
    lens = np.array([len(h) for h in hyps], dtype=np.int32)
    for i, h in enumerate(hyps):
        H[i, :len(h)] = h
        if not zero_rule:
            H[i, len(h):] = rng.integers(0, 7, L - len(h))
    if zero_rule:
        H[-1, :4] = [3, 0, 4, 5]
        assert all(edit_oracle.cut_after_zero(H[i]) == hyps[i] for i in range(N))
        assert all(edit_oracle.cut_after_zero(r) == r for R in sets for r in R)
    stats = np.array([edit_oracle.stats(h, R) for h, R in zip(hyps, sets)], dtype=np.int64)
    scores = np.array([edit_oracle.score(s) for s in stats.tolist()])
    # the fixture is not trivial: distance 0 and distance 64, the chosen reference anywhere in its set, both extremes of the score
    assert (stats[:, 0] == 0).sum() >= 5 and (stats[:, 0] == 64).sum() >= 2 and ((stats[:, 0] > 0) & (stats[:, 0] < 60)).sum() > 60
    assert set(stats[:, 3].tolist()) >= {0, 1, 2, 3, 4} and (scores == 0).sum() > 5 and (scores == 1.0).sum() >= 5
    assert {1, 5, 8} <= {len(R) for R in sets} and N >= 130
    return dict(hyps=hyps, sets=sets, H=H, lens=None if zero_rule else lens, stats=stats, scores=scores, N=N)


@pytest.fixture(scope="module")
def worlds():
    return {"zero_rule": _build(True), "lengths": _build(False)}


@pytest.fixture(scope="module")
def scorer():
    from show_edit_tell_amd import editdist
    return editdist.DeviceEditDistance(DEV)


def _wide(H, ld=72):
    """the rows inside a wider buffer: stride ld > L"""
    buf = torch.full((H.shape[0], ld), 3, dtype=torch.int64, device=DEV)
    buf[:, :H.shape[1]] = to_dev(H)
    return buf[:, :H.shape[1]]


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("rule", ["zero_rule", "lengths"])
def test_statistics_and_scores_against_oracle(worlds, scorer, rule, strided):
    w = worlds[rule]
    N = w["N"]
    refs = scorer.prepare_refs(w["sets"])
    assert (refs.n_sets, refs.L, refs.max_set) == (N, 64, 8)
    H = _wide(w["H"]) if strided else to_dev(w["H"])
    assert H.stride(0) == (72 if strided else 64)
    stats, scores = scorer.score_token_ids(H, np.arange(N), refs, hyp_lens=w["lens"])
    assert stats.dtype == torch.int32 and scores.dtype == torch.float64 and stats.is_cuda and scores.is_cuda
    assert tuple(stats.shape) == (N, 4) and tuple(scores.shape) == (N,)
    assert np.array_equal(stats.cpu().numpy(), w["stats"])
    err = np.abs(scores.cpu().numpy() - w["scores"]).max()
    _report("score_abs_err_%s" % rule, err)
    assert err <= TOL
    got = scorer.corpus_score(H, np.arange(N), refs, hyp_lens=w["lens"])
    want = edit_oracle.corpus(zip(w["hyps"], w["sets"]))
    assert sorted(got) == ["similarity", "wer"] and want["wer"] > 0.3
    for k in got:
        assert got[k].is_cuda and got[k].dtype == torch.float64 and got[k].dim() == 0
        err = abs(float(got[k]) - want[k])
        _report("corpus_%s_abs_err" % k, err)
        assert err <= TOL


def test_rows_of_one_id(scorer):
    """L = 1 on both sides: the hypothesis tensor has one column, the records one position"""
    H = to_dev(np.array([[4], [0], [5], [4]], dtype=np.int64))
    sets = [[[4]], [[0], [4]], [[4], [5]], [[6]]]
    refs = scorer.prepare_refs(sets)
    assert refs.L == 1
    stats, scores = scorer.score_token_ids(H, [0, 1, 2, 3], refs)
    assert stats.cpu().tolist() == [[0, 1, 1, 0], [0, 1, 1, 0], [0, 1, 1, 1], [1, 1, 1, 0]]
    assert scores.cpu().tolist() == [1.0, 1.0, 1.0, 0.0]
    stats, scores = scorer.score_token_ids(H, [0, 1, 2, 3], refs, hyp_lens=[1, 0, 1, 5])
    assert stats.cpu().tolist() == [[0, 1, 1, 0], [1, 0, 1, 0], [0, 1, 1, 1], [1, 1, 1, 0]]
    assert scores.cpu().tolist() == [1.0, 0.0, 1.0, 0.0]


def _raw(scorer, H, lens, set_of, refs, stats, scores, pairs, pair_ld, max_set=None, n_sets=None):
    from show_edit_tell_amd import _lib
    rc = scorer._lib.set_edit_device_score(H.data_ptr(), H.stride(0), None if lens is None else lens.data_ptr(), H.shape[0],
                                           H.shape[1], set_of.data_ptr(), refs.recs.data_ptr(), refs.L, refs.n_refs,
                                           refs.set_off.data_ptr(), refs.n_sets if n_sets is None else n_sets,
                                           refs.max_set if max_set is None else max_set, stats.data_ptr(),
                                           None if scores is None else scores.data_ptr(),
                                           None if pairs is None else pairs.data_ptr(), pair_ld, _lib.stream_of(scorer.dev))
    _lib.check(rc, "set_edit_device_score")


def _guarded(n, dtype, fill, G=16):
    return torch.full((n + 2 * G,), fill, dtype=dtype, device=DEV)


def _run_guarded(scorer, H, lens, so, refs, ld, **kw):
    """one raw launch into pre-filled buffers with guard words: (stats (n, 4), scores (n,), pairs (n, ld)) on the host, the
    guards checked"""
    n, G = H.shape[0], 16
    st, sc, pr = _guarded(n * 4, torch.int32, SENT_I), _guarded(n, torch.float64, SENT_F), _guarded(n * ld, torch.float64, SENT_F)
    _raw(scorer, H, lens, so, refs, st[G:], sc[G:], pr[G:], ld, **kw)
    out = []
    for buf, m, sent in ((st.cpu(), n * 4, SENT_I), (sc.cpu(), n, SENT_F), (pr.cpu(), n * ld, SENT_F)):
        assert (buf[:G] == sent).all() and (buf[G + m:] == sent).all()
        out.append(buf[G:G + m])
    return out[0].view(n, 4), out[1], out[2].view(n, ld)


@pytest.mark.parametrize("rule", ["zero_rule", "lengths"])
def test_launch_independence_and_guards(worlds, scorer, rule):
    """a row alone and in a batch of 130: the same bits; only stats[0..n), scores[0..n) and pair_scores[i, r < |set|] are
    written (strided rows; under `lengths`, junk behind the explicit lengths)"""
    w = worlds[rule]
    N, ld = 130, 11
    first = w["N"] - N                                             # the last 130 rows: edge cases and sets of 8 included
    refs = scorer.prepare_refs(w["sets"])
    H, so = _wide(w["H"]), torch.arange(w["N"], dtype=torch.int32, device=DEV)
    ln = None if w["lens"] is None else to_dev(w["lens"])
    rows = slice(first, first + N)
    cut = lambda a: None if ln is None else ln[a]
    st, sc, pr = _run_guarded(scorer, H[rows], cut(rows), so[rows], refs, ld)
    size = torch.tensor([len(R) for R in w["sets"][rows]])
    written = torch.arange(ld)[None, :] < size[:, None]
    assert (pr[~written] == SENT_F).all() and torch.isfinite(pr[written]).all() and (pr[written] != SENT_F).all()
    assert np.array_equal(st.numpy(), w["stats"][rows])
    assert np.abs(sc.numpy() - w["scores"][rows]).max() <= TOL
    sizes = size.tolist()
    for i in (0, 1, 64, sizes.index(8), N - 1):
        one = slice(first + i, first + i + 1)
        st1, sc1, pr1 = _run_guarded(scorer, H[one], cut(one), so[one], refs, ld)
        assert torch.equal(st1[0], st[i]), i
        assert torch.equal(sc1.view(torch.int64)[0], sc.view(torch.int64)[i]), i
        assert torch.equal(pr1[0].view(torch.int64), pr[i].view(torch.int64)), i
    # scores == NULL and pair_scores == NULL: the statistics alone
    st2 = _guarded(N * 4, torch.int32, SENT_I)
    _raw(scorer, H[rows], cut(rows), so[rows], refs, st2[16:], None, None, 0)
    assert torch.equal(st2.cpu()[16:16 + N * 4].view(N, 4), st)


def test_what_the_host_cannot_check(worlds, scorer):
    """a set index outside [0, n_sets) or a set larger than max_set: -1 / NaN in that row alone, its pair scores untouched,
    the neighbours correct, nothing outside the declared outputs written"""
    w = worlds["lengths"]
    n = 6
    sizes = [len(R) for R in w["sets"]]
    five = sizes.index(5)
    refs = scorer.prepare_refs(w["sets"])
    pick = [2, five, 7, 0, five + 2, 4]                            # rows; their sets below
    H, ln = to_dev(w["H"][pick]), to_dev(w["lens"][pick])
    so = torch.tensor([2, five, -1, refs.n_sets, five + 2, 4], dtype=torch.int32, device=DEV)
    assert sizes[2] == 1 and sizes[4] == 1 and sizes[five + 2] == 5
    st, sc, pr = _run_guarded(scorer, H, ln, so, refs, 9)
    for i in (2, 3):
        assert (st[i] == -1).all() and torch.isnan(sc[i]) and (pr[i] == SENT_F).all()
    for i in (0, 1, 4, 5):
        assert st[i].tolist() == w["stats"][pick[i]].tolist() and abs(float(sc[i]) - w["scores"][pick[i]]) <= TOL
        assert torch.isfinite(pr[i, :sizes[pick[i]]]).all() and (pr[i, sizes[pick[i]]:] == SENT_F).all()
    # the caller's bound on the set size is 4: the sets of 5 are refused, the sets of 1 scored
    so = torch.tensor(pick, dtype=torch.int32, device=DEV)
    st, sc, pr = _run_guarded(scorer, H, ln, so, refs, 9, max_set=4)
    for i in range(n):
        if sizes[pick[i]] > 4:
            assert (st[i] == -1).all() and torch.isnan(sc[i]) and (pr[i] == SENT_F).all()
        else:
            assert st[i].tolist() == w["stats"][pick[i]].tolist() and abs(float(sc[i]) - w["scores"][pick[i]]) <= TOL
    assert sum(s > 4 for s in (sizes[p] for p in pick)) == 3


def test_the_id_limit(scorer):
    """65533 is an id like any other; 65534 inside a sentence gives -1 / NaN in exactly the rows that read it"""
    big, over = 65533, 65534
    hyps = [[1, big, 2, 3], [1, 2, 3], [big, big], [4, 5, 6], [1, 2, 3]]
    sets = [[[big, 2, 9], [1, big]], [[1, 2, 3, 4]], [[big], [big, 7, big]], [[4, 6]]]
    H = np.zeros((5, 6), dtype=np.int64)
    for i, h in enumerate(hyps):
        H[i, :len(h)] = h
    lens = [len(h) for h in hyps]
    set_of = [0, 1, 2, 3, 0]
    want = [edit_oracle.stats(h, sets[s]) for h, s in zip(hyps, set_of)]
    assert want[0] == [2, 4, 3, 0] and want[2] == [1, 2, 3, 1]     # 1/2 twice: the first; 2/3 beats 1/2
    stats, scores = scorer.score_token_ids(to_dev(H), set_of, scorer.prepare_refs(sets, count_end=False), hyp_lens=lens)
    assert stats.cpu().tolist() == want
    assert np.abs(scores.cpu().numpy() - np.array([edit_oracle.score(s) for s in want])).max() <= TOL
    # in a hypothesis: that row alone; behind its length it is not part of the sentence
    Hb = H.copy()
    Hb[1, 1] = over
    Hb[3, 5] = over
    stats, scores, pairs = scorer.score_token_ids(to_dev(Hb), set_of, scorer.prepare_refs(sets, count_end=False), hyp_lens=lens,
                                                  return_pairs=True)
    stats, scores, pairs = stats.cpu(), scores.cpu(), pairs.cpu()
    assert (stats[1] == -1).all() and torch.isnan(scores[1]) and torch.isnan(pairs[1, 0]) and pairs[1, 1] == 0
    keep = [0, 2, 3, 4]
    assert stats[keep].tolist() == [want[i] for i in keep] and torch.isfinite(scores[keep]).all()
    # in a reference: the rows of that set (0 and 4)
    bad_sets = [[list(r) for r in R] for R in sets]
    bad_sets[0][1][0] = over
    stats, scores = scorer.score_token_ids(to_dev(H), set_of, scorer.prepare_refs(bad_sets, count_end=False), hyp_lens=lens)
    stats, scores = stats.cpu(), scores.cpu()
    assert (stats[[0, 4]] == -1).all() and torch.isnan(scores[[0, 4]]).all()
    assert stats[1:4].tolist() == want[1:4] and torch.isfinite(scores[1:4]).all()


def test_limits(scorer):
    from show_edit_tell_amd._lib import SetError
    refs = scorer.prepare_refs([[[1, 0]]])
    with pytest.raises(SetError):
        scorer.score_token_ids(torch.zeros(2, 65, dtype=torch.int64, device=DEV), [0, 0], refs)
    with pytest.raises(ValueError):
        scorer.prepare_refs([[[1] * 65]])
    with pytest.raises(ValueError):
        scorer.prepare_refs([[[1, 2]], []])                       # an empty set
    stats, scores = scorer.score_token_ids(torch.zeros(0, 5, dtype=torch.int64, device=DEV), [], refs)
    assert tuple(stats.shape) == (0, 4) and tuple(scores.shape) == (0,)
    got = scorer.corpus_score(torch.zeros(0, 5, dtype=torch.int64, device=DEV), [], refs)
    assert float(got["similarity"]) == 0.0 and float(got["wer"]) == 0.0


@pytest.mark.parametrize("rule", ["zero_rule", "lengths"])
def test_pair_scores(worlds, scorer, rule):
    w = worlds[rule]
    rows = np.arange(w["N"] - 130, w["N"])
    sets = [w["sets"][i] for i in rows]
    lens = None if w["lens"] is None else w["lens"][rows]
    refs = scorer.prepare_refs(sets)
    stats, scores, pairs = scorer.score_token_ids(_wide(w["H"][rows]), np.arange(len(rows)), refs, hyp_lens=lens, return_pairs=True)
    pairs = pairs.cpu().numpy()
    assert pairs.shape == (len(rows), 8)
    err = 0.0
    for a, i in enumerate(rows):
        want = [edit_oracle.sentence(w["hyps"][i], [r]) for r in w["sets"][i]]
        err = max([err] + [abs(pairs[a, r] - x) for r, x in enumerate(want)])
        assert not pairs[a, len(want):].any()                     # beyond the set: the zeros of the allocation
    _report("pair_abs_err", err)
    assert err <= TOL
    assert np.array_equal(stats.cpu().numpy(), w["stats"][rows])


def _consensus_fixture():
    """3 images x 5 candidates of 12..14 ids: candidate 2 of every image is the sentence the others are one- or two-word
    mutations of, so it is the closest to all the others"""
    rng = np.random.default_rng(33)
    cands = []
    for i in range(3):
        base = [int(w) for w in rng.integers(1, 40, 13)]
        for j in range(5):
            c = list(base)
            if j != 2:
                c[(3 * j + i) % 13] = 40 + j
                if j % 2:
                    c = c[:12] if j == 1 else c + [45]
            cands.append(c + [0])
    return cands


def test_consensus_rerank_under_the_edit_similarity(scorer):
    from show_edit_tell_amd import editdist
    from show_edit_tell_amd.evaluate import consensus_rerank
    cands = _consensus_fixture()
    T = np.zeros((15, 20), dtype=np.int64)
    for i, c in enumerate(cands):
        T[i, :len(c)] = c
    S, host = np.zeros((3, 5, 5)), editdist.EditDistance()
    for i in range(3):
        for j in range(5):
            for r in range(5):
                S[i, j, r] = edit_oracle.sentence(cands[i * 5 + j], [cands[i * 5 + r]])
                assert S[i, j, r] == host.score_from_stats(host.sentence_stats(cands[i * 5 + j], [cands[i * 5 + r]]))
    P = scorer.pair_scores(to_dev(T), 5)
    assert tuple(P.shape) == (15, 5) and np.abs(P.cpu().numpy().reshape(3, 5, 5) - S).max() <= TOL
    want = np.zeros((3, 5))
    for i in range(3):
        for j in range(5):
            want[i, j] = np.mean([S[i, j, r] for r in range(5) if r != j])
    srt = np.sort(want, 1)
    margin = (srt[:, -1] - srt[:, -2]).min()
    print("consensus margin of the best candidate: %.4f" % margin)
    assert margin > 1e-6 and want.argmax(1).tolist() == [2, 2, 2]
    best, util = consensus_rerank(scorer, to_dev(T), 5)
    err = np.abs(util.cpu().numpy() - want).max()
    _report("consensus_abs_err", err)
    assert err <= TOL and best.cpu().tolist() == want.argmax(1).tolist()


def test_records_are_shared_with_bleu(worlds, scorer):
    """DeviceBleu.prepare_refs and DeviceEditDistance.prepare_refs write the same bytes, and either scores under both scorers"""
    import bleu_oracle
    from show_edit_tell_amd import bleu
    w = worlds["zero_rule"]
    rows = slice(w["N"] - 40, w["N"])
    sets, H, N = w["sets"][rows], to_dev(w["H"][rows]), 40
    bscorer = bleu.DeviceBleu(DEV)
    for count_end in (True, False):
        rb, rr = bscorer.prepare_refs(sets, count_end=count_end), scorer.prepare_refs(sets, count_end=count_end)
        assert torch.equal(rb.recs, rr.recs) and torch.equal(rb.set_off, rr.set_off)
        assert (rb.L, rb.n_refs, rb.n_sets, rb.max_set) == (rr.L, rr.n_refs, rr.n_sets, rr.max_set)
    want_b = np.array([bleu_oracle.stats(h, R) for h, R in zip(w["hyps"][rows], sets)])
    for refs in (bscorer.prepare_refs(sets), scorer.prepare_refs(sets)):
        st, sc = scorer.score_token_ids(H, np.arange(N), refs)
        assert np.array_equal(st.cpu().numpy(), w["stats"][rows]) and np.abs(sc.cpu().numpy() - w["scores"][rows]).max() <= TOL
        st, _ = bscorer.score_token_ids(H, np.arange(N), refs)
        assert np.array_equal(st.cpu().numpy(), want_b)
