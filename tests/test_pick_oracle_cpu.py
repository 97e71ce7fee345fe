"""CPU: tests/pick_oracle.py — the numpy restatements that judge the pick kernels — against torch-CPU (log_softmax, LSTMCell),
against the reference loop's bookkeeping written out step by step, and against oracle/beam_np.beam_loop."""
import numpy as np
import torch

import pick_oracle as PO
from oracle import beam_np


def test_greedy_words_match_torch_log_softmax_and_first_index():
    rng = np.random.default_rng(0)
    for B, V, n in ((5, 7, 1), (3, 257, 3), (2, 1025, 6)):
        slabs = rng.integers(-8, 9, size=(n, B, V + 3)).astype(np.float32)
        bias = rng.integers(-8, 9, size=V).astype(np.float32)
        x = PO.slab_logits(slabs, bias, V)
        want = torch.from_numpy(slabs[:, :, :V]).double().sum(0) + torch.from_numpy(bias).double()
        assert np.array_equal(x, want.numpy())
        ls = torch.log_softmax(want, 1)
        words, logp = PO.greedy_words(x)
        for b in range(B):
            first = int(torch.nonzero(want[b] == want[b].max())[0, 0])           # integer logits: real ties, the first one wins
            assert words[b] == first
            assert abs(logp[b] - float(ls[b, first])) < 1e-12
    assert (PO.slab_logits(slabs, None, V) == slabs[:, :, :V].astype(np.float64).sum(0)).all()


def test_greedy_words_on_degenerate_rows():
    nan, inf = np.nan, np.inf
    x = np.array([[nan, nan, nan, nan], [-inf, -inf, -inf, -inf], [1.0, nan, 3.0, 3.0], [-inf, 2.0, -inf, 2.0], [nan, -inf, nan, -inf]])
    words, logp = PO.greedy_words(x)
    assert words.tolist() == [0, 0, 2, 1, 0]
    assert np.isnan(logp[[0, 1, 2, 4]]).all() and abs(logp[3] + np.log(2.0)) < 1e-15


def test_bookkeeping_matches_the_reference_loop_written_out():
    """editnet_rl.py:517-547 line by line on scripted picks, against book_step / greedy_step"""
    rng = np.random.default_rng(1)
    B, V, max_len, end = 6, 9, 5, 8
    x = rng.integers(-8, 9, size=(max_len + 2, B, V)).astype(np.float64)
    x[2, :, end] = 50.0                                              # every row ends at t = 2: the loop is left after it
    x[1, 0, 0] = 40.0                                                # row 0 picks word 0 (not <end>) at t = 1: it latches
    st = PO.new_state(B, max_len, fill=-3)
    seq, seq_logp = np.full((B, max_len), -3, np.int64), np.full((B, max_len), -3.0)
    unfinished, left = None, False
    for t in range(max_len + 2):
        PO.greedy_step(x[t], t, max_len, end, st)
        if left or t >= max_len:
            continue
        lp = torch.log_softmax(torch.from_numpy(x[t]), 1)
        val, it = lp.max(1)
        it = it.numpy().copy()
        it[it == end] = 0
        unfinished = (it > 0) if t == 0 else unfinished & (it > 0)
        it = it * unfinished
        seq[:, t], seq_logp[:, t] = it, val.numpy()
        assert np.array_equal(st["it"], it) and np.array_equal(st["unf"], unfinished.astype(np.int32))
        assert st["alive"][t] == unfinished.sum()
        left = unfinished.sum() == 0
    assert left and np.array_equal(st["seq"], seq) and np.abs(st["seq_logp"] - seq_logp).max() < 1e-12
    assert (seq[:, 3:] == -3).all() and seq[0, 1] == 0 and st["alive"].tolist()[3:] == [0] * (max_len - 1)
    # the row limit: <end> at t + 1 >= limit whatever the scores say, the log-prob stays the arg-max's
    st2 = PO.new_state(2, 3)
    y = np.array([[0.0, 5.0, 1.0, 0.0], [0.0, 1.0, 5.0, 0.0]])
    assert PO.greedy_step(y, 0, 3, 3, st2, row_limit=[1, 2]).tolist() == [3, 2]
    assert st2["it"].tolist() == [0, 2] and st2["unf"].tolist() == [0, 1]
    assert abs(st2["seq_logp"][0, 0] - float(torch.log_softmax(torch.from_numpy(y), 1)[0, 1])) < 1e-12


def test_relu_embed_and_lstm_tail_match_torch():
    rng = np.random.default_rng(2)
    E = rng.standard_normal((7, 8)).astype(np.float32)
    it = np.array([0, 6, 3])
    assert np.array_equal(PO.relu_embed(E, it), torch.relu(torch.from_numpy(E))[it].numpy())
    for n, D, with_pre in ((1, 4, False), (3, 8, True), (4, 12, True)):
        Bn = 5
        cell = torch.nn.LSTMCell(D, D, bias=False).double()
        xin, h, c = (torch.from_numpy(rng.standard_normal((Bn, D))) for _ in range(3))
        with torch.no_grad():
            gx, gh = xin @ cell.weight_ih.T, h @ cell.weight_hh.T     # split further into n partials below
            h1, c1 = cell(xin, (h, c))
        parts = rng.standard_normal((n - 1, Bn, 4 * D))
        pre = rng.standard_normal((Bn, 4 * D)) if with_pre else None
        last = gx.numpy() - parts.sum(0) - (pre if with_pre else 0.0)
        g0 = np.concatenate([parts, last[None]], 0)
        hh, cc = PO.lstm_tail(g0, pre, gh.numpy(), c.numpy())
        assert np.abs(hh - h1.numpy()).max() < 1e-12 and np.abs(cc - c1.numpy()).max() < 1e-12


class _Scripted:
    """a beam_np state whose logits depend on the step and the word fed only (nothing to re-index)"""
    def __init__(self, table):
        self.table, self.t = table, 0

    def step(self, words):
        out = self.table[self.t][words]
        self.t += 1
        return out

    def reindex(self, idx):
        pass


def _scripted_tables(rng, steps, V, end, p_end):
    """(steps, V, V) logits: per row one word at 0, every other word at -(32 + u), u uniform in [0, 8) — the row's log-sum-exp is
    its largest logit in float32 and equal candidates do not occur"""
    tab = -(32.0 + 8.0 * rng.random((steps, V, V))).astype(np.float32)
    for s in range(steps):
        for w in range(V):
            tab[s, w, end if rng.random() < p_end else int(rng.integers(1, V - 1))] = 0.0
    tab[steps - 1, :, :] = -40.0
    tab[steps - 1, :, end] = 0.0                                     # the last step ends every hypothesis
    return tab


def test_beam_pick_matches_beam_np_beam_loop():
    rng = np.random.default_rng(3)
    for k, V, ld, p_end in ((3, 16, 16, 0.3), (5, 37, 40, 0.2), (8, 16, 19, 0.25), (1, 9, 9, 0.3)):
        end, start, steps = V - 1, V - 2, 6
        Lmax = steps + 2
        tab = _scripted_tables(rng, steps, V, end, p_end)
        assert np.float32(1.0) + np.float32(V - 1) * np.exp(np.float32(-32.0)) == np.float32(1.0)
        want_seq, want_score, _ = beam_np.beam_loop([_Scripted(tab)], lambda ls: PO.log_softmax64(ls[0]).astype(np.float32),
                                                    start, end, V, k)
        neg = np.float32(-np.inf)
        scores = np.full((1, k), neg, np.float32)
        scores[0, 0] = 0.0
        k_left, seqs = np.full(1, k, np.int32), np.full((1, k, Lmax), start, np.int64)
        best_score, best_seq, best_len = np.full(1, neg, np.float32), np.zeros((1, Lmax), np.int64), np.zeros(1, np.int32)
        done_score, done_seq = np.full((1, k), neg, np.float32), np.zeros((1, k, Lmax), np.int64)
        done_len, n_done = np.zeros((1, k), np.int32), np.zeros(1, np.int32)
        words = np.full(k, start, np.int64)
        flags = {}
        for cur_len in range(1, steps + 1):
            lg = np.full((k, ld), np.nan, np.float32)
            lg[:, :V] = tab[cur_len - 1][words]
            seqs, words, rows = PO.beam_pick(lg, scores, k_left, seqs, best_score, best_seq, best_len, done_score, done_seq,
                                             done_len, n_done, cur_len, flags, k, V, end)
            assert (rows // k == 0).all()
            if k_left[0] == 0:
                break
        assert k_left[0] == 0 and n_done[0] == k
        assert best_seq[0, :best_len[0]].tolist() == want_seq and abs(float(best_score[0]) - want_score) < 1e-5
        assert best_score[0] == done_score[0].max()
