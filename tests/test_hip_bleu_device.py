"""GPU: BLEU on the device (csrc/bleu_device.hip, bleu.DeviceBleu) against the float64 restatement tests/bleu_oracle.py:
statistics and sentence scores at every length / set-size edge under both sentence conventions, launch independence and the
memory contract, pair scores, the corpus score, validation_bleu on a beam-search output, the consensus rerank and the SCST
steps with a BLEU term.

Tolerances.  The statistics are integers: equality.  A sentence or corpus score lies in [0, 1) and is a product of four
quotients, one pow and one exp in double, a few ulp each (under 1e-14 relative): 1e-9 absolute is asserted, the bound the
project asserts for device CIDEr-D.  Rewards are float32 of magnitude below 10: 2 ulp of 10 (1.9e-6), the loss 1e-5
relative, as tests/test_hip_ciderd_device.py::test_scst_step_device_reward_matches_host asserts them; the same 1e-5, relative
to the largest magnitude of a tensor, is asked of the updated parameters."""
import json
import os

import numpy as np
import pytest
import torch

import bleu_oracle
from hip_adapter import dcnet_modules, editnet_modules, to_dev

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL, TOL_REWARD, TOL_REL = 1e-9, 1.9e-6, 1e-5
SENT_I, SENT_F = -777, -12345.678
LENGTHS = (5, 64, 0, 1, 2, 3, 4, 63)            # row i has length LENGTHS[i % 8]: row 0 is an ordinary one
MEASURED = {}


def _report(name, value):
    """the measured maxima, printed and (SET_BLEU_ERRORS_OUT=file) collected for profiles/bleu_device_errors.json"""
    MEASURED[name] = max(float(value), MEASURED.get(name, 0.0))
    print("measured %s = %.3e" % (name, value))
    out = os.environ.get("SET_BLEU_ERRORS_OUT")
    if out:
        with open(out, "w") as f:
            json.dump(MEASURED, f, indent=1, sort_keys=True)


def _build(zero_rule):
    """257 hypotheses over the ids 1..6, each with its own set of 1..5 references.  Reference lengths rotate through 1, 3, 64
    and l -/+ 1, l -/+ 2, l (l = the hypothesis length), so sets of two and more hold pairs at equal distance on both sides.
    Half of the references are mutated copies of the hypothesis (long grams match, counts clip), half are random.
    zero_rule: sentences end with the token 0 (rows are cut after their first 0) — except row 1, a full row of 64 ids without
    0; otherwise rows carry explicit lengths and junk (0s included) behind them."""
    rng = np.random.default_rng(7 if zero_rule else 8)

    def words(n):
        return [int(w) for w in rng.integers(1, 7, n)]

    hyps, sets = [], []
    for i in range(257):
        l = LENGTHS[i % 8]
        h = words(l)
        if zero_rule:
            if l == 0:
                h = [0]
            elif i != 1:
                h[-1] = 0
        pool = [1, 3, 64, l - 1, l + 1, l - 2, l + 2, l]
        start = (i // 8) % len(pool)
        refs = []
        for j in range(1 + i % 5):
            n = min(64, max(0, pool[(start + j) % len(pool)]))
            if (i + j) % 2 == 0 and len(h) > 0:
                body = [w for w in h if w] or [1]
                r = [body[a % len(body)] for a in range(n)]
                for _ in range(int(rng.integers(0, 3))):
                    if n:
                        r[int(rng.integers(0, n))] = int(rng.integers(1, 7))
            else:
                r = words(n)
            if zero_rule and n and j % 2 == 0:
                r[-1] = 0
            refs.append(r)
        hyps.append(h)
        sets.append(refs)
    L = 64
    H = np.zeros((257, L), dtype=np.int64)
    lens = np.array([len(h) for h in hyps], dtype=np.int32)
    for i, h in enumerate(hyps):
        H[i, :len(h)] = h
        if not zero_rule:
            H[i, len(h):] = rng.integers(0, 7, L - len(h))
    if zero_rule:
        assert 0 not in H[1] and all(bleu_oracle.cut_after_zero(H[i]) == hyps[i] for i in range(257))
    stats = np.array([bleu_oracle.stats(h, R) for h, R in zip(hyps, sets)], dtype=np.int64)
    scores = np.array([bleu_oracle.score(s) for s in stats.tolist()])
    # the fixture is not trivial: clipping, full matches of order 4, a tie of the closest length on both sides of a hypothesis
    assert ((stats[:, 0:4] < stats[:, 4:8]).any(1) & (stats[:, 0] > 0)).sum() > 100 and (stats[:, 3] > 0).sum() > 40
    ties = [i for i, (h, R) in enumerate(zip(hyps, sets))
            if any(len(a) < len(h) < len(b) and len(h) - len(a) == len(b) - len(h) == abs(stats[i, 9] - len(h)) for a in R for b in R)]
    assert len(ties) >= 8 and all(stats[i, 9] < stats[i, 8] for i in ties)
    assert {1, 3, 64} <= {len(r) for R in sets for r in R} and {len(R) for R in sets} == {1, 2, 3, 4, 5}
    return dict(hyps=hyps, sets=sets, H=H, lens=None if zero_rule else lens, stats=stats, scores=scores)


@pytest.fixture(scope="module")
def worlds():
    return {"zero_rule": _build(True), "lengths": _build(False)}


@pytest.fixture(scope="module")
def scorer():
    from show_edit_tell_amd import bleu
    return bleu.DeviceBleu(DEV)


def _wide(H, ld=72):
    """the rows inside a wider buffer: stride ld > L"""
    buf = torch.full((H.shape[0], ld), 3, dtype=torch.int64, device=DEV)
    buf[:, :H.shape[1]] = to_dev(H)
    return buf[:, :H.shape[1]]


@pytest.mark.parametrize("N", [1, 5, 65, 257])
@pytest.mark.parametrize("rule", ["zero_rule", "lengths"])
def test_statistics_and_scores_against_oracle(worlds, scorer, rule, N):
    w = worlds[rule]
    refs = scorer.prepare_refs(w["sets"][:N])
    assert (refs.n_sets, refs.L, refs.max_set) == (N, 64 if N > 1 else max(len(r) for r in w["sets"][0]), min(N, 5))
    H = _wide(w["H"][:N])
    assert H.stride(0) == 72
    stats, scores = scorer.score_token_ids(H, np.arange(N), refs, hyp_lens=None if w["lens"] is None else w["lens"][:N])
    assert stats.dtype == torch.int32 and scores.dtype == torch.float64 and stats.is_cuda and scores.is_cuda
    assert tuple(stats.shape) == (N, 10) and tuple(scores.shape) == (N, 4)
    assert np.array_equal(stats.cpu().numpy(), w["stats"][:N])
    err = np.abs(scores.cpu().numpy() - w["scores"][:N]).max()
    _report("score_abs_err_%s" % rule, err)
    assert err <= TOL


def _raw(scorer, H, lens, set_of, refs, stats, scores, pairs, pair_ld):
    from show_edit_tell_amd import _lib
    rc = scorer._lib.set_bleu_device_score(H.data_ptr(), H.stride(0), None if lens is None else lens.data_ptr(), H.shape[0],
                                           H.shape[1], set_of.data_ptr(), refs.recs.data_ptr(), refs.L, refs.n_refs,
                                           refs.set_off.data_ptr(), refs.n_sets, refs.max_set, stats.data_ptr(),
                                           None if scores is None else scores.data_ptr(),
                                           None if pairs is None else pairs.data_ptr(), pair_ld, _lib.stream_of(scorer.dev))
    _lib.check(rc, "set_bleu_device_score")


def _guarded(n, dtype, fill, G=16):
    return torch.full((n + 2 * G,), fill, dtype=dtype, device=DEV)


def test_launch_independence_and_guards(worlds, scorer):
    """row 0 alone and in the batch of 257: the same bits; only stats[0..N), scores[0..N) and pair_scores[i, r < |set|] are
    written (guard words around all three and around the reference records, the tail of short sets)"""
    from show_edit_tell_amd import _lib
    w = worlds["zero_rule"]
    N, G, ld = 257, 16, 7
    # the reference records: written inside their bytes only
    flat = [r for R in w["sets"] for r in R]
    tok = np.zeros((len(flat), 64), dtype=np.int64)
    for i, r in enumerate(flat):
        tok[i, :len(r)] = r
    ln = to_dev(np.array([len(r) for r in flat], dtype=np.int32))
    words = len(flat) * (8 + 4 * 64)
    assert scorer._lib.set_bleu_device_ref_bytes(len(flat), 64) == words * 8
    rbuf = _guarded(words, torch.int64, SENT_I)
    tk = to_dev(tok)
    _lib.check(scorer._lib.set_bleu_device_prepare(tk.data_ptr(), 64, ln.data_ptr(), len(flat), 64, rbuf[G:].data_ptr(),
                                                   _lib.stream_of(scorer.dev)), "set_bleu_device_prepare")
    refs = scorer.prepare_refs(w["sets"])
    rb = rbuf.cpu()
    assert (rb[:G] == SENT_I).all() and (rb[G + words:] == SENT_I).all()
    assert torch.equal(rb[G:G + words], refs.recs.cpu())

    H, so = _wide(w["H"]), torch.arange(N, dtype=torch.int32, device=DEV)

    def run(rows):
        n = rows.stop - rows.start
        st, sc, pr = _guarded(n * 10, torch.int32, SENT_I), _guarded(n * 4, torch.float64, SENT_F), _guarded(n * ld, torch.float64, SENT_F)
        _raw(scorer, H[rows], None, so[rows], refs, st[G:], sc[G:], pr[G:], ld)
        out = []
        for buf, m, sent in ((st.cpu(), n * 10, SENT_I), (sc.cpu(), n * 4, SENT_F), (pr.cpu(), n * ld, SENT_F)):
            assert (buf[:G] == sent).all() and (buf[G + m:] == sent).all()
            out.append(buf[G:G + m])
        return out[0].view(n, 10), out[1].view(n, 4), out[2].view(n, ld)
    st, sc, pr = run(slice(0, N))
    again = run(slice(0, N))
    assert torch.equal(st, again[0]) and torch.equal(sc.view(torch.int64), again[1].view(torch.int64))
    assert torch.equal(pr.view(torch.int64), again[2].view(torch.int64))
    size = torch.tensor([len(R) for R in w["sets"]])
    written = torch.arange(ld)[None, :] < size[:, None]
    assert (pr[~written] == SENT_F).all() and torch.isfinite(pr[written]).all() and (pr[written] != SENT_F).all()
    assert np.array_equal(st.numpy(), w["stats"])
    for i in (0, 1, 2, 100, 256):
        st1, sc1, pr1 = run(slice(i, i + 1))
        assert torch.equal(st1[0], st[i]), i
        assert torch.equal(sc1[0].view(torch.int64), sc[i].view(torch.int64)), i
        assert torch.equal(pr1[0].view(torch.int64), pr[i].view(torch.int64)), i
    # scores == NULL: the statistics alone
    st2 = _guarded(N * 10, torch.int32, SENT_I)
    _raw(scorer, H, None, so, refs, st2[G:], None, None, 0)
    assert torch.equal(st2.cpu()[G:G + N * 10].view(N, 10), st)


def test_what_the_host_cannot_check(worlds, scorer):
    """a set index outside [0, n_sets): -1 / NaN in that row alone; an id the packing cannot hold: NaN in that row alone"""
    w = worlds["zero_rule"]
    refs = scorer.prepare_refs(w["sets"][:8])
    H = to_dev(w["H"][:4])
    bad = torch.tensor([2, -1, 8, 3], dtype=torch.int32, device=DEV)
    stats, scores, pairs = scorer.score_token_ids(H, bad, refs, return_pairs=True)
    stats, scores, pairs = stats.cpu(), scores.cpu(), pairs.cpu()
    assert (stats[1] == -1).all() and (stats[2] == -1).all() and torch.isnan(scores[1:3]).all() and not pairs[1:3].any()
    assert (stats[0] >= 0).all() and (stats[3] >= 0).all() and torch.isfinite(scores[0]).all() and torch.isfinite(scores[3]).all()
    big = H.clone()
    big[0, 0] = 65534
    stats, scores = scorer.score_token_ids(big, [0, 1, 2, 3], refs)
    assert torch.isnan(scores[0]).all() and torch.isfinite(scores[1:]).all() and (stats[0, :4] == -1).all()
    assert np.array_equal(stats[1:].cpu().numpy(), w["stats"][1:4])


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
    assert tuple(stats.shape) == (0, 10) and tuple(scores.shape) == (0, 4)


@pytest.mark.parametrize("rule", ["zero_rule", "lengths"])
def test_pair_scores_and_corpus_score(worlds, scorer, rule):
    w = worlds[rule]
    rows = np.arange(0, 257, 3)
    sets = [w["sets"][i] for i in rows]
    lens = None if w["lens"] is None else w["lens"][rows]
    refs = scorer.prepare_refs(sets)
    stats, scores, pairs = scorer.score_token_ids(_wide(w["H"][rows]), np.arange(len(rows)), refs, hyp_lens=lens, return_pairs=True)
    pairs = pairs.cpu().numpy()
    assert pairs.shape == (len(rows), 5)
    err = 0.0
    for a, i in enumerate(rows):
        want = [bleu_oracle.sentence(w["hyps"][i], [r])[3] for r in w["sets"][i]]
        err = max([err] + [abs(pairs[a, r] - x) for r, x in enumerate(want)])
        assert not pairs[a, len(want):].any()                     # beyond the set: the zeros of the allocation
    _report("pair_abs_err", err)
    assert err <= TOL
    want = np.array(bleu_oracle.corpus((w["hyps"][i], w["sets"][i]) for i in rows))
    got = scorer.corpus_score(_wide(w["H"][rows]), np.arange(len(rows)), refs, hyp_lens=lens)
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (4,)
    err = np.abs(got.cpu().numpy() - want).max()
    _report("corpus_abs_err", err)
    assert err <= TOL
    assert np.abs(want - scores.cpu().numpy().mean(0)).min() > 1e-3      # not the mean of the sentence scores


def test_validation_bleu_on_a_beam_search_output():
    """the small DCNet: batched beam search (token lists) and the greedy decode (an id tensor) through validation_bleu against
    bleu.Bleu on the same ids read back, both conventions"""
    from show_edit_tell_amd import bleu, ciderd, evaluate
    d, _, rl = dcnet_modules("dcnet_small")
    wm = d["wm"]
    prev, plen = to_dev(d["prev"]), to_dev(d["plen"])
    seqs = evaluate.beam_search_dcnet_batched(rl, prev, plen, wm, 3, max_steps=8)
    with torch.no_grad():
        greedy, _ = rl(wm, prev, plen, sample_max=True, sample_rl=False)
    B = len(seqs)
    drop, end = {int(wm["<start>"]), int(wm["<pad>"])}, int(wm["<end>"])
    ids = [[0 if t == end else int(t) for t in s if int(t) not in drop] for s in seqs]
    rng = np.random.default_rng(5)
    gt = []
    for b in range(B):                                            # the search's own words, perturbed: the scores are not zeros
        body = [t for t in ids[b] if t] or [1]
        refs = []
        for j in range(3):
            r = list(body)
            r[int(rng.integers(0, len(r)))] = int(rng.integers(1, len(wm) - 4))
            refs.append(r[:len(r) - j % 2] + [0])
        gt.append(refs)
    host = bleu.Bleu()
    for count_end in (False, True):
        rows = ids if count_end else [[t for t in s if t] for s in ids]
        refs = gt if count_end else bleu.strip_end(gt)
        T = np.zeros((B, max(len(r) for r in rows) + 1), dtype=np.int64)
        for b, r in enumerate(rows):
            T[b, :len(r)] = r
        want = host.corpus_from_stats(host.score_token_ids(T, np.arange(B), refs, hyp_lens=[len(r) for r in rows])[0])
        got = evaluate.validation_bleu(seqs, None, gt, DEV, count_end=count_end, word_map=wm)
        assert got.is_cuda and tuple(got.shape) == (4,)
        err = np.abs(got.cpu().numpy() - np.array(want)).max()
        _report("validation_abs_err", err)
        assert err <= TOL and want[0] > 0.1
        # the greedy tensor: the decoder's format as it is
        g = greedy.cpu().numpy()
        if count_end:
            st, _ = host.score_token_ids(g, np.arange(B), gt)
        else:
            glen = [int(np.flatnonzero(r == 0)[0]) if (r == 0).any() else len(r) for r in g]
            st, _ = host.score_token_ids(g, np.arange(B), refs, hyp_lens=glen)
        got = evaluate.validation_bleu(greedy, None, gt, DEV, count_end=count_end)
        assert np.abs(got.cpu().numpy() - np.array(host.corpus_from_stats(st))).max() <= TOL


def _consensus_fixture():
    """3 images x 5 candidates of 12..14 ids: candidate 2 of every image is the sentence the others are one- or two-word
    mutations of, so it has the largest mean BLEU-4 against the others"""
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


def test_consensus_rerank_under_bleu(scorer):
    from show_edit_tell_amd.evaluate import consensus_rerank, consensus_rerank_lists
    cands = _consensus_fixture()
    T = np.zeros((15, 20), dtype=np.int64)
    for i, c in enumerate(cands):
        T[i, :len(c)] = c
    S = np.zeros((3, 5, 5))
    for i in range(3):
        for j in range(5):
            for r in range(5):
                S[i, j, r] = bleu_oracle.sentence(cands[i * 5 + j], [cands[i * 5 + r]])[3]
    P = scorer.pair_scores(to_dev(T), 5)
    assert tuple(P.shape) == (15, 5) and np.abs(P.cpu().numpy().reshape(3, 5, 5) - S).max() <= TOL
    w = np.array([[0.4, 0.1, 0.2, 0.2, 0.1], [1, 1, 1, 1, 1], [0.5, 0.5, 0.0, 0.5, 0.0]])
    for weights in (None, w):
        ww = np.ones((3, 5)) if weights is None else weights
        want = np.zeros((3, 5))
        for i in range(3):
            for j in range(5):
                others = [r for r in range(5) if r != j]
                den = sum(ww[i, r] for r in others)
                want[i, j] = sum(ww[i, r] * S[i, j, r] for r in others) / den if den else 0.0
        srt = np.sort(want, 1)
        margin = (srt[:, -1] - srt[:, -2]).min()
        print("consensus margin of the best candidate: %.4f" % margin)
        assert margin > 0.02 and want.argmax(1).tolist() == [2, 2, 2]        # unique, and far above the 1e-9 of the scores
        best, util = consensus_rerank(scorer, to_dev(T), 5, weights)
        err = np.abs(util.cpu().numpy() - want).max()
        _report("consensus_abs_err", err)
        assert err <= TOL and best.cpu().tolist() == [2, 2, 2]
        assert tuple(util.shape) == (3, 5) and util.is_cuda and best.dtype == torch.int64
    b2, u2 = consensus_rerank_lists(scorer, [cands[0:5], cands[5:10], cands[10:15]])
    plain = consensus_rerank(scorer, to_dev(T), 5)[1].cpu().numpy()
    assert b2 == [2, 2, 2] and np.abs(np.array(u2) - plain).max() <= TOL


def test_reward_mix_against_host(scorer):
    """self_critical_reward_device with a BLEU term against self_critical_reward: 8 images x 3 samples"""
    from show_edit_tell_amd import bleu, ciderd
    rng = np.random.default_rng(8)
    gt = [[[int(w) for w in rng.integers(1, 58, int(rng.integers(5, 12)))] + [0] for _ in range(5)] for _ in range(8)]
    df, docs = ciderd.document_frequency([[ciderd.tokens_to_str(c) for c in caps] for caps in gt])
    sc = ciderd.CiderD(df, docs)

    def near(b):
        c = [w for w in gt[b][int(rng.integers(0, 5))] if w][:18]
        c[int(rng.integers(0, len(c)))] = int(rng.integers(1, 58))
        row = np.zeros(20, dtype=np.int64)
        row[:len(c)] = c
        return row
    greedy = np.stack([near(b) for b in range(8)])
    sampled = np.stack([near(b % 8) for b in range(24)])
    want = ciderd.self_critical_reward(sc, sampled, np.tile(greedy, (3, 1)), gt * 3, 0.7, bleu.Bleu(), 0.5)
    only_c = ciderd.self_critical_reward(sc, sampled, np.tile(greedy, (3, 1)), gt * 3, 0.7)
    assert np.abs(want - only_c).max() > 0.05                    # the BLEU term is there
    dsc = sc.device(DEV)
    got = ciderd.self_critical_reward_device(dsc, to_dev(sampled), to_dev(greedy), dsc.prepare_refs(gt), None, 0.7,
                                             scorer, scorer.prepare_refs(gt), 0.5)
    assert got.dtype == torch.float32 and tuple(got.shape) == (24, 20) and got.is_cuda
    err = np.abs(got.cpu().numpy().astype(np.float64) - want.astype(np.float64)).max()
    _report("reward_abs_err", err)
    assert err <= TOL_REWARD
    again = ciderd.self_critical_reward_device(dsc, to_dev(sampled), to_dev(greedy), gt, None, 0.7, scorer, gt, 0.5)
    assert torch.equal(again, got)


def _scst_refs(wm, B, model_greedy):
    """the set-up of tests/test_hip_ciderd_device.py: 5 random captions per image over the real vocabulary — and the model's
    own greedy caption as the first, so that rewards are not all zero"""
    from show_edit_tell_amd import ciderd
    V = len(wm)
    rng = np.random.default_rng(3)
    allcaps = np.zeros((B, 5, 24), dtype=np.int64)
    for b in range(B):
        for j in range(5):
            n = int(rng.integers(3, 9))
            words = rng.integers(1, V - 4, n)
            if j == 0:
                g = [int(w) for w in model_greedy[b] if int(w) > 0][:20]
                words = np.array(g if g else [1], dtype=np.int64)
                n = len(words)
            allcaps[b, j, 0] = wm["<start>"]
            allcaps[b, j, 1:1 + n] = words
            allcaps[b, j, 1 + n] = wm["<end>"]
    gt = ciderd.ground_truth_lists(allcaps, wm)
    df, docs = ciderd.document_frequency([[ciderd.tokens_to_str(c) for c in caps] for caps in gt])
    return gt, ciderd.CiderD(df, max(docs, 2))


def _scst_run(net, **kw):
    from show_edit_tell_amd import train
    if net == "editnet":
        d, _, rl = editnet_modules("editnet_small")
        inputs = (to_dev(d["X"]), to_dev(d["prev"]), to_dev(d["plen"]))
        greedy_in = (to_dev(d["prev"]), to_dev(d["plen"]), to_dev(d["X"]))
        step = train.scst_train_step
    else:
        d, _, rl = dcnet_modules("dcnet_small")
        inputs = (to_dev(d["prev"]), to_dev(d["plen"]))
        greedy_in = inputs
        step = train.dcnet_scst_train_step
    wm = d["wm"]
    with torch.no_grad():
        g, _ = rl(wm, *greedy_in, sample_max=True, sample_rl=False)
    gt, scorer = _scst_refs(wm, inputs[0].shape[0], g.cpu().numpy())
    opt = torch.optim.Adam(rl.parameters(), lr=1e-3)
    torch.manual_seed(4)
    out = step(rl, opt, wm, *inputs, gt, scorer, n_samples=3, **kw)
    params = [p.detach().cpu().clone() for p in rl.parameters()]
    assert all(torch.isfinite(p).all() for p in params)
    return out, params


@pytest.mark.parametrize("net", ["editnet", "dcnet"])
def test_scst_step_with_bleu_term_device_matches_host(net):
    """two identical models and seeds, one step each with reward="host" and reward="device", bleu_weight = 0.5"""
    (r_h, l_h), p_h = _scst_run(net, reward="host", bleu_weight=0.5)
    (r_d, l_d), p_d = _scst_run(net, reward="device", bleu_weight=0.5)
    (r_0, _), _ = _scst_run(net, reward="host")
    print("reward host %.9g device %.9g (without the BLEU term %.9g), loss host %.9g device %.9g" % (r_h, r_d, r_0, l_h, l_d))
    _report("scst_%s_reward_abs_diff" % net, abs(r_h - r_d))
    _report("scst_%s_loss_rel_diff" % net, abs(l_h - l_d) / max(abs(l_h), 1e-30))
    par = max(float((a - b).abs().max() / a.abs().max().clamp_min(1e-30)) for a, b in zip(p_h, p_d))
    _report("scst_%s_param_rel_diff" % net, par)
    assert np.isfinite([r_h, l_h, r_d, l_d]).all()
    assert abs(r_h - r_0) > 1e-3                                  # the BLEU term moved the reward
    assert abs(r_h - r_d) <= TOL_REWARD
    assert abs(l_h - l_d) <= TOL_REL * abs(l_h)
    assert par <= TOL_REL


@pytest.mark.parametrize("net", ["editnet", "dcnet"])
@pytest.mark.parametrize("route", ["host", "device"])
def test_scst_step_bleu_weight_zero_is_the_step_without_it(net, route):
    (r_a, l_a), p_a = _scst_run(net, reward=route)
    (r_b, l_b), p_b = _scst_run(net, reward=route, bleu_weight=0.0)
    assert r_a == r_b and l_a == l_b
    assert all(torch.equal(a, b) for a, b in zip(p_a, p_b))
