"""CPU: cocoEval's `CIDEr` on the host — ciderd.corpus_cider and CiderD.from_corpus (df and N from the reference sets of the
corpus that is scored) against two values computed by hand and against tests/cider_oracle.py on the world of
tests/test_hip_rouge_validation.py.  Tolerance against the oracle: both sides are double sums of at most 4 orders x 5
references x 19 grams of terms <= 1, in different orders, times 10: a few hundred ulp of 10 at the very most, 1e-12 asserted."""
import math

import numpy as np
import pytest

import cider_oracle

TOL = 1e-12


def _s(ids):
    return " ".join(str(int(w)) for w in ids)


def _gts_res(hyps, sets):
    gts = {i: [_s(r) for r in refs] for i, refs in enumerate(sets)}
    res = [{"image_id": i, "caption": [_s(h)]} for i, h in enumerate(hyps)]
    return gts, res


def test_two_images_score_five_by_hand():
    """references [[1, 2]] and [[1, 3]], hypotheses [1, 2] and [1, 3]; N = 2.  Unigram 1 is in both sets: idf log 2 - log 2 = 0.
    Order 1: the vectors {1: 0, 2: log 2} are equal, similarity 1.  Order 2: one bigram with df 1 on both sides, similarity 1.
    Orders 3 and 4 are empty: 0.  Equal lengths: penalty 1.  (1 + 1 + 0 + 0) / 4 * 10 = 5, exactly."""
    from show_edit_tell_amd import ciderd
    sets, hyps = [[[1, 2]], [[1, 3]]], [[1, 2], [1, 3]]
    mean, scores = ciderd.corpus_cider(*_gts_res(hyps, sets))
    assert list(scores) == [5.0, 5.0] and mean == 5.0
    assert cider_oracle.corpus(hyps, [0, 1], sets) == (5.0, [5.0, 5.0])
    # coco's own input form for the captions
    assert ciderd.corpus_cider({0: ["1 2"], 1: ["1 3"]}, {0: ["1 2"], 1: ["1 3"]})[0] == 5.0


def test_single_image_scores_zero():
    """N = 1: log N = 0 and every df is 1, so every weight is 0 — coco-caption's 0.0 for a corpus of one image"""
    from show_edit_tell_amd import ciderd
    mean, scores = ciderd.corpus_cider(*_gts_res([[4, 5, 6]], [[[4, 5, 6], [4, 5]]]))
    assert mean == 0.0 and list(scores) == [0.0]
    assert cider_oracle.corpus([[4, 5, 6]], [0], [[[4, 5, 6], [4, 5]]]) == (0.0, [0.0])


def test_from_corpus_counts_a_gram_once_per_set():
    from show_edit_tell_amd import ciderd
    sets = [[[7, 7, 7, 8], [7, 8], [7, 7]],           # 7 three times in one reference and in all three references
            [[9, 7]],
            [[9]]]
    sc = ciderd.CiderD.from_corpus([[_s(r) for r in refs] for refs in sets])
    assert sc.ref_len == 3.0 and sc.n == 4 and sc.sigma == 6.0
    assert sc.df[("7",)] == 2 and sc.df[("9",)] == 2 and sc.df[("8",)] == 1
    assert sc.df[("7", "7")] == 1 and sc.df[("7", "8")] == 1 and sc.df[("7", "7", "7", "8")] == 1
    want = cider_oracle.document_frequency(sets)
    assert {tuple(int(w) for w in g): c for g, c in sc.df.items()} == want
    assert ciderd.CiderD.from_corpus([["1 2"]], n=2, sigma=3.0).sigma == 3.0


def test_the_world_is_the_one_the_figures_describe():
    w = cider_oracle.world()
    hyps, sets = cider_oracle.world_sides(w, False)
    df = cider_oracle.document_frequency(sets)
    assert len(sets) == 37 and len(df) == 1624 and max(df.values()) == 19
    assert round(cider_oracle.corpus(hyps, range(37), sets)[0], 3) == 3.754


@pytest.mark.parametrize("count_end", [False, True])
def test_corpus_cider_against_oracle(count_end):
    from show_edit_tell_amd import ciderd
    w = cider_oracle.world()
    hyps, sets = cider_oracle.world_sides(w, count_end)
    want_mean, want = cider_oracle.corpus(hyps, range(w["N"]), sets)
    assert 1.0 < want_mean < 8.0                      # no degenerate fixture
    gts, res = _gts_res(hyps, sets)
    mean, scores = ciderd.corpus_cider(gts, res)
    err = float(np.abs(np.asarray(scores) - np.asarray(want)).max())
    print("CIDEr %.6f (count_end=%s), max abs err %.3e" % (want_mean, count_end, err))
    assert err <= TOL and abs(mean - want_mean) <= TOL
    # the scorer object, through its public scoring call, gives the same numbers
    sc = ciderd.CiderD.from_corpus(gts.values())
    assert sc.log_ref_len == math.log(37.0)
    for i in (0, 5, 17, 36):
        assert abs(sc.score(res[i]["caption"][0], gts[i]) - want[i]) <= TOL
