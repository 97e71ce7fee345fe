"""CPU: the host side of the edit trace (show_edit_tell_amd/evaluate.py): greedy output -> forced token lists, the step
counts of ragged token lists, and the copy / edit labels of an EditTrace built from hand-made tensors."""
import numpy as np
import pytest
import torch

from show_edit_tell_amd import evaluate

WM = {"<pad>": 0, "cat": 1, "dog": 2, "sat": 3, "mat": 4, "<unk>": 5, "<start>": 6, "<end>": 7}
START, END = WM["<start>"], WM["<end>"]


def test_tokens_from_greedy_rows_ending_at_step_0_midway_and_never():
    seq = np.zeros((3, 18), np.int64)
    seq[1, :5] = [1, 2, 3, 4, 1]                      # <end> was picked at step 5 (stored as 0)
    seq[2] = np.arange(18) % 4 + 1                    # never ended: all 18 positions hold words
    want = [[START, END],
            [START, 1, 2, 3, 4, 1, END],
            [START] + seq[2].tolist()]
    assert evaluate.tokens_from_greedy(seq, WM) == want
    assert evaluate.tokens_from_greedy(torch.from_numpy(seq), WM) == want
    assert [len(r) - 1 for r in want] == [1, 6, 18]   # recorded steps: the <end> step counts, a cut row has no <end> step


def test_n_steps_from_ragged_token_lists_and_from_a_tensor_with_lengths():
    toks = [[START, 1, 2, END], [START, END], [START, 3, 4, 1, 2, 3]]
    tok, n_steps, S = evaluate._forced_tokens(toks, None, "cpu")
    assert S == 5 and tok.shape == (3, 6) and tok.dtype == torch.long
    assert n_steps.dtype == torch.int32 and n_steps.tolist() == [3, 1, 5]
    assert tok.tolist() == [[START, 1, 2, END, 0, 0], [START, END, 0, 0, 0, 0], [START, 3, 4, 1, 2, 3]]
    # the same rows as a padded tensor (junk behind the lengths is dropped) + lengths
    padded = torch.full((3, 8), 5, dtype=torch.long)
    for b, r in enumerate(toks):
        padded[b, :len(r)] = torch.tensor(r)
    tok2, n2, S2 = evaluate._forced_tokens(padded, torch.tensor([4, 2, 6]), "cpu")
    assert S2 == S and torch.equal(tok2, tok) and torch.equal(n2, n_steps)
    with pytest.raises(ValueError):
        evaluate._forced_tokens(padded, None, "cpu")
    with pytest.raises(ValueError):
        evaluate._forced_tokens([[START, 1], []], None, "cpu")
    # a lone <start> records nothing, S stays a legal step count
    tok3, n3, S3 = evaluate._forced_tokens([[START]], None, "cpu")
    assert S3 == 1 and n3.tolist() == [0] and tok3.tolist() == [[START, 0]]


def _hand_trace():
    prev = torch.tensor([[1, 2, 3, 0], [4, 4, 1, 2]])
    tokens = torch.tensor([[START, 1, 4, END, 0], [START, 4, 2, 3, END]])
    n_steps = torch.tensor([3, 4], dtype=torch.int32)
    select = torch.tensor([[0, 1, 2, -1], [1, 3, 0, 2]], dtype=torch.int32)
    gate = torch.tensor([[0.9, 0.2, 0.5, 0.0], [0.8, 0.7, 0.1, 0.3]])
    B, S, T, R, D = 2, 4, 4, 3, 8
    return evaluate.EditTrace(torch.zeros(B, S, T), select, gate, torch.zeros(B, S, D), torch.zeros(B, S, R),
                              torch.zeros(B, S), n_steps, tokens, prev)


def test_copied_labels_with_a_padded_tail():
    tr = _hand_trace()
    # row 0: "cat" == prev[0] copied; "mat" vs prev[1] = "dog" edited; <end> vs prev[2] edited; tail select = -1 never copied
    # row 1: "mat" == prev[1]; "dog" == prev[3]; "sat" vs prev[0] = "mat" edited; <end> vs prev[2] edited
    want = torch.tensor([[True, False, False, False], [True, True, False, False]])
    assert tr.copied.dtype == torch.bool and torch.equal(tr.copied, want)
    # a padded step is never a copy, even where token 0 would equal a <pad> of the previous caption
    tr.previous_caption[0, 3] = 0
    assert not bool(tr.copied[0, 3])


def test_rows_lists_only_recorded_steps():
    rows = _hand_trace().rows(WM)
    assert [len(r) for r in rows] == [3, 4]
    assert rows[0] == [("cat", "cat", pytest.approx(0.9), True), ("mat", "dog", pytest.approx(0.2), False),
                       ("<end>", "sat", pytest.approx(0.5), False)]
    assert rows[1][1] == ("dog", "dog", pytest.approx(0.7), True)
    assert rows[1][3] == ("<end>", "cat", pytest.approx(0.3), False)
