"""CPU: rouge.RougeL (the host statement of coco-caption's ROUGE-L) against the independent restatement tests/rouge_oracle.py on
a fixed-seed grid, hand-worked cases with their integers written out, coco's calling forms, the 0 rule — and the 64-bit
bit-parallel recurrence that csrc/rouge_device.hip runs, stated here in Python integers, against the oracle's table."""
import numpy as np
import pytest

import rouge_oracle

MASK64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def scorer():
    from show_edit_tell_amd import rouge
    return rouge.RougeL()


@pytest.fixture(scope="module")
def grid():
    g = rouge_oracle.grid()
    assert {len(h) for h, _ in g} == {0, 1, 2, 7, 63, 64} and {len(R) for _, R in g} == {1, 5}
    assert {len(r) for _, R in g for r in R} >= {0, 1, 2, 7, 63, 64}
    return g


def test_grid_against_oracle(scorer, grid):
    nonzero = 0
    for h, R in grid:
        st = scorer.sentence_stats(h, R)
        assert st == rouge_oracle.stats(h, R), (h, R)
        got, want = scorer.score_from_stats(st), rouge_oracle.score(st)
        assert isinstance(got, float) and got == want, (h, R, got, want)           # the same operations in the same order
        assert 0.0 <= got <= 1.0
        nonzero += got > 0
    assert nonzero > len(grid) // 3


def test_beta_squared_is_one_product():
    """the oracle squares beta as a product, coco as a power: the same double for 1.2"""
    assert 1.2 * 1.2 == 1.2 ** 2


def test_hand_worked_cases(scorer):
    b2 = 1.2 * 1.2
    # identical: P = Rc = 1, and (1 + b2) / (1 + b2) is exactly 1
    assert scorer.sentence_stats([4, 5, 6], [[4, 5, 6]]) == [3, 3, 3, 3]
    assert scorer.score_from_stats([3, 3, 3, 3]) == 1.0
    # disjoint
    assert scorer.sentence_stats([1, 2, 3], [[4, 5], [6]]) == [0, 3, 0, 2]
    assert scorer.score_from_stats([0, 3, 0, 2]) == 0.0
    # the best precision and the best recall come from different references
    st = scorer.sentence_stats([1, 2, 3, 4, 5, 6], [[1, 2], [1, 2, 3, 9, 9, 9, 9, 9, 9, 9]])
    assert st == [3, 6, 2, 2]
    P, Rc = 3 / 6, 2 / 2
    assert scorer.score_from_stats(st) == (1.0 + b2) * P * Rc / (Rc + b2 * P)
    # a subsequence, not a substring: 1 . 3 . 5
    assert scorer.sentence_stats([1, 2, 3, 4, 5], [[1, 9, 3, 8, 5, 7]]) == [3, 5, 3, 6]
    # equal recalls 2/4 and 3/6: the first reference stays; and in the other order
    assert scorer.sentence_stats([1, 2, 3], [[1, 2, 8, 8], [1, 2, 3, 9, 9, 9]]) == [3, 3, 2, 4]
    assert scorer.sentence_stats([1, 2, 3], [[1, 2, 3, 9, 9, 9], [1, 2, 8, 8]]) == [3, 3, 3, 6]
    # an empty hypothesis
    assert scorer.sentence_stats([], [[1, 2]]) == [0, 0, 0, 2] and scorer.score_from_stats([0, 0, 0, 2]) == 0.0
    # an empty reference beside another: skipped; alone or all empty: (0, 0) and the score 0
    assert scorer.sentence_stats([1, 2], [[], [2, 3]]) == [1, 2, 1, 2]
    assert scorer.sentence_stats([1, 2], [[]]) == [0, 2, 0, 0]
    assert scorer.sentence_stats([1, 2], [[], [], []]) == [0, 2, 0, 0] and scorer.score_from_stats([0, 2, 0, 0]) == 0.0
    # an empty reference never wins the recall, even against recall 0
    assert scorer.sentence_stats([1, 2], [[], [7, 8, 9]]) == [0, 2, 0, 3]
    for st in ([3, 3, 3, 3], [0, 3, 0, 2], [3, 6, 2, 2], [3, 5, 3, 6], [0, 2, 0, 0], [1, 2, 1, 2]):
        assert scorer.score_from_stats(st) == rouge_oracle.score(st)


def test_beta_is_checked():
    from show_edit_tell_amd import rouge
    for beta in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            rouge.RougeL(beta)
    assert rouge.RougeL(2.0).score_from_stats([1, 2, 1, 4]) == rouge_oracle.score([1, 2, 1, 4], 2.0)


def test_zero_rule_with_and_without_lengths(scorer):
    H = np.array([[5, 6, 0, 7, 0], [5, 0, 6, 7, 8], [1, 2, 3, 4, 8]])
    sets = [[[5, 6, 0, 9], [6, 7, 0]], [[5, 0, 6, 7]]]
    # without lengths: rows and references are cut after their first 0, which stays a token
    stats, scores = scorer.score_token_ids(H, [0, 1, 0], sets)
    assert stats.dtype == np.int64 and stats.shape == (3, 4) and scores.dtype == np.float64 and scores.shape == (3,)
    assert stats.tolist() == [[3, 3, 3, 3], [2, 2, 2, 2], [0, 5, 0, 3]]
    assert scores[0] == 1.0 and scores[1] == 1.0 and scores[2] == 0.0
    # with lengths: exactly that long, a 0 inside the sentence is a token like any other
    stats, scores = scorer.score_token_ids(H, [0, 1, 1], sets, hyp_lens=[5, 4, 9])
    want0 = rouge_oracle.stats([5, 6, 0, 7, 0], [[5, 6, 0], [6, 7, 0]])
    assert want0 == [3, 5, 3, 3] and stats[0].tolist() == want0
    assert stats[1].tolist() == rouge_oracle.stats([5, 0, 6, 7], [[5, 0]]) == [2, 4, 2, 2]
    assert stats[2].tolist() == [0, 5, 0, 2]                              # the length is clamped to the row
    assert scores[0] == rouge_oracle.score(want0)
    stats, _ = scorer.score_token_ids(H, [0, 1, 1], sets, hyp_lens=[0, -3, 2])
    assert stats[:, 1].tolist() == [0, 0, 2]
    with pytest.raises(ValueError):
        scorer.score_token_ids(H, [0, 1], sets)
    with pytest.raises(ValueError):
        scorer.score_token_ids(H[0], [0], sets)


def test_compute_score_in_both_forms(scorer):
    gts = {"a": ["the cat sat on the mat", "a cat sat"], "b": ["dogs bark"], 7: ["one two three four"]}
    caps = {"a": ["the cat is on the mat"], "b": ["cats purr loudly"], 7: ["two four"]}
    want = [rouge_oracle.sentence(caps[k][0].split(), [s.split() for s in gts[k]]) for k in ("a", "b", 7)]
    assert want[0] > 0.5 and want[1] == 0.0 and want[2] > 0.0
    mean, per = scorer.compute_score(gts, caps)
    assert per == want and mean == float(np.mean(want))
    as_list = [{'image_id': k, 'caption': caps[k]} for k in (7, "a", "b")]
    mean2, per2 = scorer.compute_score(gts, as_list)
    assert per2 == [want[2], want[0], want[1]] and abs(mean2 - mean) < 1e-15
    # the mean of the sentence scores, not a score of summed statistics
    tot = np.sum([scorer.sentence_stats(caps[k][0].split(), [s.split() for s in gts[k]]) for k in ("a", "b", 7)], 0)
    assert abs(scorer.score_from_stats(tot) - mean) > 1e-3


def bit_parallel_lcs(h, r):
    """The recurrence of csrc/rouge_device.hip in Python integers: bit i of a word is position i of the reference (lane i),
    fields are id + 1 and 0 beyond the length; V starts at all ones, one step per hypothesis position, the carry out of bit
    63 is dropped; LCS = the number of cleared bits."""
    assert len(h) <= 64 and len(r) <= 64
    g = [x + 1 for x in r] + [0] * (64 - len(r))
    V = MASK64
    for x in h:
        f = x + 1
        M = sum(1 << i for i in range(64) if g[i] == f)
        U = V & M
        V = ((V + U) & MASK64) | (V & ~M & MASK64)
    return 64 - bin(V).count("1")


def test_bit_parallel_recurrence_against_the_table(grid):
    n = 0
    for h, R in grid:
        for r in R:
            assert bit_parallel_lcs(h, r) == rouge_oracle.lcs(h, r), (h, r)
            assert bit_parallel_lcs(r, h) == rouge_oracle.lcs(h, r), (r, h)
            n += 1
    assert n > 500
    full = list(range(64))
    assert bit_parallel_lcs(full, full) == 64                              # every bit of V cleared
    assert bit_parallel_lcs([3] * 64, [3] * 64) == 64 and bit_parallel_lcs([3] * 64, [3] * 63) == 63
    assert bit_parallel_lcs(full, full[::-1]) == 1 == rouge_oracle.lcs(full, full[::-1])
    assert bit_parallel_lcs([0, 0], [0]) == 1                              # the id 0 is a token: its field is 1


def test_module_is_numpy_only_at_import():
    import subprocess
    import sys
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); import show_edit_tell_amd.rouge as r; assert 'torch' not in sys.modules; "
            "print(r.RougeL().score_from_stats([1, 1, 1, 1]))" % root)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "1.0", out.stderr
