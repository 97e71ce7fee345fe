"""CPU: the word edit distance of editdist.py (the host scorer, the canonical alignment) against the independent restatement
tests/edit_oracle.py, the 64-bit recurrence of csrc/editdist_device.hip in Python integers against the textbook table, and
evaluate.source_rows on CPU tensors against the list rule of ciderd.ground_truth_lists."""
import random

import numpy as np
import pytest
import torch

import edit_oracle

LENGTHS = (0, 1, 2, 31, 32, 33, 63, 64)


@pytest.fixture(scope="module")
def cases():
    return edit_oracle.grid() + edit_oracle.edge_cases()


def test_host_scorer_equals_oracle_on_the_grid(cases):
    from show_edit_tell_amd import editdist
    sc = editdist.EditDistance()
    assert len(cases) >= 200
    for h, R in cases:
        st = sc.sentence_stats(h, R)
        assert st == edit_oracle.stats(h, R)
        assert sc.score_from_stats(st) == edit_oracle.score(st)
        assert editdist.distance(h, R[0]) == edit_oracle.dist(h, R[0]) == editdist.distance_table(h, R[0])[len(h)][len(R[0])]
    want = edit_oracle.corpus(cases)
    L = 64
    H = np.zeros((len(cases), L), dtype=np.int64)
    for i, (h, _) in enumerate(cases):
        H[i, :len(h)] = h
    got = sc.corpus_score(H, np.arange(len(cases)), [R for _, R in cases], hyp_lens=[len(h) for h, _ in cases])
    assert abs(got["similarity"] - want["similarity"]) <= 1e-12 and got["wer"] == want["wer"] and want["wer"] > 0


@pytest.mark.parametrize("A", [1, 2, 50])
def test_bit_parallel_recurrence_equals_the_table(A):
    rng = random.Random(100 + A)
    for lr in LENGTHS:
        for lc in LENGTHS:
            rows = [rng.randint(1, A) for _ in range(lr)]
            cols = [rng.randint(1, A) for _ in range(lc)]
            if A == 50 and lr > 2 and lc > 2:                      # a large alphabet: let a common stretch match
                n = min(lr, lc) // 2
                cols[:n] = rows[lr - n:]
            T = edit_oracle.table(rows, cols)
            d, hist = edit_oracle.bit_parallel(rows, cols)
            assert d == T[lr][lc], (A, lr, lc)
            for i in sorted({0, 1, lr // 2, max(lr - 1, 0), lr}):
                for j in sorted({0, 1, lc // 2, max(lc - 1, 0), lc}):
                    if i <= lr and j <= lc:
                        assert edit_oracle.cell(hist, i, j) == T[i][j], (A, lr, lc, i, j)


def test_every_cell_from_the_stored_columns():
    rng = random.Random(9)
    for lr, lc, A in ((64, 64, 2), (63, 64, 3), (64, 33, 6), (7, 20, 2)):
        rows, cols = [rng.randint(1, A) for _ in range(lr)], [rng.randint(1, A) for _ in range(lc)]
        T = edit_oracle.table(rows, cols)
        _, hist = edit_oracle.bit_parallel(rows, cols)
        assert all(edit_oracle.cell(hist, i, j) == T[i][j] for i in range(lr + 1) for j in range(lc + 1))


def test_alignments_equal_the_oracle_and_keep_the_identities(cases):
    from show_edit_tell_amd import editdist
    for h, R in cases:
        for src in R[:2]:
            ho, hs, so, (keep, sub, ins, dele) = editdist.alignment(src, h)
            assert (ho, hs, so, [keep, sub, ins, dele]) == edit_oracle.script(src, h)
            assert keep + sub + ins == len(h) and keep + sub + dele == len(src)
            assert sub + ins + dele == edit_oracle.dist(src, h)
            assert [k for k in hs if k >= 0] == sorted(set(k for k in hs if k >= 0))       # monotone, one source word each
            assert all((op == editdist.INS) == (k < 0) for op, k in zip(ho, hs))
            assert all(src[k] == w for op, k, w in zip(ho, hs, h) if op == editdist.KEEP)


def test_known_small_scripts():
    from show_edit_tell_amd.editdist import alignment
    a, b, c, x = 5, 6, 7, 9
    assert alignment([a, b, c], [a, x, c]) == ([1, 2, 1], [0, 1, 2], [1, 2, 1], (2, 1, 0, 0))
    assert alignment([a, c], [a, b, c]) == ([1, 3, 1], [0, -1, 1], [1, 1], (2, 0, 1, 0))             # a pure insertion
    assert alignment([a, b, c], [a, c]) == ([1, 1], [0, 2], [1, 3, 1], (2, 0, 0, 1))                 # a pure deletion
    assert alignment([], []) == ([], [], [], (0, 0, 0, 0))
    assert alignment([], [a, b]) == ([3, 3], [-1, -1], [], (0, 0, 2, 0))
    assert alignment([a, b], []) == ([], [], [3, 3], (0, 0, 0, 2))
    # of equal-cost scripts the canonical one: from the end, a diagonal step before an insertion before a deletion
    assert alignment([a, a], [a]) == ([1], [1], [3, 1], (1, 0, 0, 1))
    assert alignment([a], [a, a]) == ([3, 1], [-1, 0], [1], (1, 0, 1, 0))


def test_similarity_and_ties():
    from show_edit_tell_amd.editdist import EditDistance
    sc = EditDistance()
    assert sc.sentence_stats([], [[]]) == [0, 0, 0, 0] and sc.score_from_stats([0, 0, 0, 0]) == 1.0
    assert sc.sentence_stats([], [[1, 2], [], [3]]) == [0, 0, 0, 1]
    assert sc.sentence_stats([1, 2], [[]]) == [2, 2, 0, 0] and sc.score_from_stats([2, 2, 0, 0]) == 0.0
    # 1/2 four ways, with different denominators: the first stays; a later larger one wins
    h = [1, 2, 3, 4]
    R = [[1, 2, 9, 4, 5, 6, 7, 8], [1, 2], [5, 2, 3, 6], [1, 2, 3, 4, 5, 6, 7, 8]]
    assert sc.sentence_stats(h, R) == [2, 4, 2, 1]
    assert sc.sentence_stats(h, R + [[1, 2, 3]]) == [1, 4, 3, 4]
    assert sc.score_from_stats([1, 4, 3, 4]) == 3.0 / 4.0
    with pytest.raises(ValueError):
        sc.score_token_ids(np.array([[1, 2]]), [0], [[]])


def test_both_sentence_conventions():
    from show_edit_tell_amd.editdist import EditDistance
    sc = EditDistance()
    H = np.array([[3, 4, 0, 5, 0], [3, 4, 5, 6, 7], [0, 3, 0, 0, 0]])
    sets = [[[3, 4, 0, 9], [3, 0]], [[3, 4, 5]]]
    st, s = sc.score_token_ids(H, [0, 1, 0], sets)                 # the 0 rule: cut after the first 0, which stays
    assert st.tolist() == [[0, 3, 3, 0], [2, 5, 3, 0], [1, 1, 2, 1]] and s.tolist() == [1.0, 3.0 / 5.0, 0.5]
    st, s = sc.score_token_ids(H, [0, 1, 0], sets, hyp_lens=[4, 9, -1])            # explicit lengths, clamped to [0, L]
    assert st.tolist() == [[1, 4, 3, 0], [2, 5, 3, 0], [3, 0, 3, 0]]               # no word: 0/3 and 0/2 tie, the first stays
    out = sc.align_token_ids(H, np.array([[3, 4, 0, 7], [4, 5, 0, 0], [0, 0, 0, 0]]))
    assert out[0].tolist() == [[0, 3, 3, 3, 0, 0, 0, 1], [3, 5, 3, 2, 1, 2, 0, 0], [0, 1, 1, 1, 0, 0, 0, 1]]
    assert out[1].dtype == np.int8 and out[2].dtype == np.int32 and out[3].dtype == np.int8
    assert out[1].shape == (3, 5) and out[3].shape == (3, 4)
    assert out[1][0].tolist() == [1, 1, 1, 0, 0] and out[2][0].tolist() == [0, 1, 2, -1, -1] and out[3][0].tolist() == [1, 1, 1, 0]
    out = sc.align_token_ids(H, np.array([[3, 4, 0, 7], [4, 5, 0, 0], [0, 0, 0, 0]]), hyp_lens=[2, 2, 0], src_lens=[4, 2, 0])
    assert out[0].tolist() == [[2, 2, 4, 2, 0, 0, 2, 0], [2, 2, 2, 0, 2, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 1]]


def _toy_word_map():
    wm = {"<pad>": 0, "<unk>": 1, "<start>": 2, "<end>": 3}
    wm.update({"w%d" % k: k for k in range(4, 40)})
    return wm


def test_source_rows_follow_the_list_rule():
    """evaluate.source_rows on CPU tensors: <start> / <pad> dropped, <end> -> 0 (ciderd.ground_truth_lists), then the two
    conventions' lengths"""
    from show_edit_tell_amd import ciderd, evaluate
    wm = _toy_word_map()
    S, E, P = wm["<start>"], wm["<end>"], wm["<pad>"]
    prev = torch.tensor([[S, 5, 6, 7, E, P, P, P],
                         [S, 9, E, P, P, P, P, P],
                         [S, E, P, P, P, P, P, P],
                         [S, 4, 5, 6, 7, 8, 9, E],
                         [S, 4, P, 5, S, 6, E, 7],                 # pad and start in the middle: dropped, the rest moves up
                         [S, 4, 5, 6, 7, 8, 9, 10]])               # never ended
    plen = torch.tensor([[5], [3], [2], [8], [8], [8]])
    want = ciderd.ground_truth_lists(prev[:, None, :], wm)
    for count_end in (False, True):
        rows, lens = evaluate.source_rows(prev, plen, wm, count_end)
        assert rows.dtype == torch.int64 and lens.dtype == torch.int32 and tuple(rows.shape) == (6, 8)
        for b in range(6):
            full = want[b][0]
            cut = full[:full.index(0) + (1 if count_end else 0)] if 0 in full else full
            assert rows[b, :int(lens[b])].tolist() == cut, (b, count_end)
            assert rows[b, :len(full)].tolist() == full
    # prev_caplen bounds the row: what lies behind it is not part of the caption
    rows, lens = evaluate.source_rows(prev[4:5], torch.tensor([4]), wm)
    assert rows[0, :int(lens[0])].tolist() == [4, 5]
    rows, lens = evaluate.source_rows(prev, None, wm)
    assert lens.tolist() == [3, 1, 0, 6, 3, 7]
