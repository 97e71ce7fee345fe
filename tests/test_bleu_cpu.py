"""CPU: the host BLEU scorer (show_edit_tell_amd/bleu.py Bleu) against hand-checked statistics and against the independent
restatement tests/bleu_oracle.py."""
import numpy as np
import pytest

import bleu_oracle

# hypothesis, references, correct[1..4] + guess[1..4] + [testlen, reflen]
PINS = [
    ([1, 2, 3, 4, 5], [[1, 2, 3, 4, 5]], [5, 4, 3, 2, 5, 4, 3, 2, 5, 5]),
    ([7, 7, 7], [[7, 8]], [1, 0, 0, 0, 3, 2, 1, 0, 3, 2]),                               # the clipping
    ([7, 7, 7], [[7, 8], [7, 7, 9, 9]], [2, 1, 0, 0, 3, 2, 1, 0, 3, 2]),                 # max over references; tie -> shorter
]


@pytest.mark.parametrize("h,R,want", PINS)
def test_hand_checked_statistics(h, R, want):
    from show_edit_tell_amd.bleu import Bleu
    assert bleu_oracle.stats(h, R) == want
    assert Bleu.sentence_stats(h, R) == want
    st, sc = Bleu().score_token_ids(np.array([h + [0]]), [0], [R], hyp_lens=[len(h)])
    assert st.dtype == np.int64 and sc.dtype == np.float64 and st.shape == (1, 10) and sc.shape == (1, 4)
    assert st[0].tolist() == want


def test_identical_sentence_scores_just_under_one():
    from show_edit_tell_amd.bleu import Bleu
    for got in (bleu_oracle.sentence([1, 2, 3, 4, 5], [[1, 2, 3, 4, 5]]), Bleu.scores_from_stats(PINS[0][2])):
        assert all(1.0 - 1e-8 < x < 1.0 for x in got)


def test_empty_hypothesis_scores_zero():
    from show_edit_tell_amd.bleu import Bleu
    assert bleu_oracle.sentence([], [[7, 8]]) == [0.0] * 4
    st, sc = Bleu().score_token_ids(np.zeros((1, 3), dtype=np.int64), [0], [[[7, 8]]], hyp_lens=[0])
    assert st[0].tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 0, 2] and sc[0].tolist() == [0.0] * 4


def test_guess_zero_contributes_1e_minus_6():
    """h = [7, 8] against itself: orders 3 and 4 have no gram, each multiplies b by 1e-15 / 1e-9"""
    got = bleu_oracle.sentence([7, 8], [[7, 8]])
    pen = np.exp(1 - 1 / ((2 + 1e-15) / (2 + 1e-9)))
    assert got[2] == pytest.approx((1e-6) ** (1 / 3) * pen, rel=1e-6)
    assert got[3] == pytest.approx((1e-12) ** (1 / 4) * pen, rel=1e-6)


@pytest.fixture(scope="module")
def random_rows():
    rng = np.random.default_rng(2024)
    hyps, sets = [], []
    for _ in range(200):
        hyps.append([int(w) for w in rng.integers(1, 7, int(rng.integers(0, 21)))])
        sets.append([[int(w) for w in rng.integers(1, 7, int(rng.integers(0, 21)))] for _ in range(int(rng.integers(1, 6)))])
    return hyps, sets


def test_random_sentences_against_oracle(random_rows):
    from show_edit_tell_amd.bleu import Bleu
    hyps, sets = random_rows
    H = np.full((200, 20), 9, dtype=np.int64)                # what lies behind the length is not read
    for i, h in enumerate(hyps):
        H[i, :len(h)] = h
    st, sc = Bleu().score_token_ids(H, np.arange(200), sets, hyp_lens=[len(h) for h in hyps])
    want_st = np.array([bleu_oracle.stats(h, R) for h, R in zip(hyps, sets)])
    clipped = ((want_st[:, 0:4] < want_st[:, 4:8]).any(1) & (want_st[:, 0] > 0)).sum()
    assert clipped > 100, clipped                             # the fixture is not trivial
    assert np.array_equal(st, want_st)
    want_sc = np.array([bleu_oracle.score(s) for s in want_st.tolist()])
    assert np.all(np.abs(sc - want_sc) <= 1e-12 * np.abs(want_sc))
    # the corpus score sums the statistics: not the mean of the sentence scores
    corp = Bleu.corpus_from_stats(st)
    want_corp = bleu_oracle.corpus(zip(hyps, sets))
    assert np.all(np.abs(np.array(corp) - np.array(want_corp)) <= 1e-12 * np.array(want_corp))
    assert all(abs(c - m) > 1e-3 for c, m in zip(corp, sc.mean(0)))


def test_zero_rule_of_the_rows():
    """lens=None: a row ends after its first 0 and the 0 is a token; a row without 0 is taken whole; references are cut alike"""
    from show_edit_tell_amd.bleu import Bleu
    H = np.array([[3, 4, 0, 5, 6], [3, 4, 5, 6, 7], [0, 3, 3, 3, 3]])
    refs = [[[3, 4, 0, 9, 9], [4]]]
    st, _ = Bleu().score_token_ids(H, [0, 0, 0], refs)
    assert st.tolist() == [bleu_oracle.stats([3, 4, 0], [[3, 4, 0], [4]]), bleu_oracle.stats([3, 4, 5, 6, 7], [[3, 4, 0], [4]]),
                           bleu_oracle.stats([0], [[3, 4, 0], [4]])]
    assert st[0].tolist() == [3, 2, 1, 0, 3, 2, 1, 0, 3, 3]


def test_compute_score_on_strings_equals_token_ids(random_rows):
    from show_edit_tell_amd.bleu import Bleu
    hyps, sets = random_rows
    hyps, sets = hyps[:40], sets[:40]
    words = {i: w for i, w in enumerate("zero a man riding wave on the".split())}
    say = lambda ids: " ".join(words[i] for i in ids)
    gts = {i: [say(r) for r in R] for i, R in enumerate(sets)}
    res_list = [{'image_id': i, 'caption': [say(h)]} for i, h in enumerate(hyps)]
    res_dict = {i: [say(h)] for i, h in enumerate(hyps)}
    H = np.zeros((40, 20), dtype=np.int64)
    for i, h in enumerate(hyps):
        H[i, :len(h)] = h
    st, sc = Bleu().score_token_ids(H, np.arange(40), sets, hyp_lens=[len(h) for h in hyps])
    for res in (res_list, res_dict):
        corp, per = Bleu().compute_score(gts, res)
        assert corp == Bleu.corpus_from_stats(st)
        assert len(per) == 4 and all(per[k] == sc[:, k].tolist() for k in range(4))


def test_corpus_from_stats_accepts_torch():
    import torch
    from show_edit_tell_amd.bleu import Bleu
    st = np.array([PINS[1][2], PINS[2][2], PINS[0][2]])
    want = Bleu.corpus_from_stats(st)
    assert want == bleu_oracle.score(st.sum(0).tolist())
    got = Bleu.corpus_from_stats(torch.from_numpy(st).to(torch.int32))
    assert got.dtype == torch.float64 and tuple(got.shape) == (4,)
    assert np.all(np.abs(got.numpy() - np.array(want)) <= 1e-12 * np.array(want))


def test_refusals():
    from show_edit_tell_amd.bleu import Bleu
    with pytest.raises(ValueError):
        Bleu(n=2)
    with pytest.raises(ValueError):
        Bleu().score_token_ids(np.zeros((1, 3), dtype=np.int64), [0], [[]])          # a hypothesis without reference
    with pytest.raises(ValueError):
        Bleu().score_token_ids(np.zeros((2, 3), dtype=np.int64), [0], [[[1]]])
