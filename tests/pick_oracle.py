"""Plain numpy restatements of the vocabulary-row epilogues (csrc/epilogue.hip greedy_pick_k / sample_pick_k with their
LstmTail, csrc/beam.hip beam_pick_k), used by tests/test_hip_pick_epilogues.py and tests/test_hip_nbest_beam.py.
tests/test_pick_oracle_cpu.py pins them to torch-CPU (log_softmax, LSTMCell) and to oracle/beam_np.beam_loop, so no GPU test
leans on an unchecked helper."""
import numpy as np


def slab_logits(slabs, bias, V):
    """(n, B, >= V) partials (+ bias (V)) -> (B, V) float64 logits"""
    x = np.asarray(slabs, np.float64)[:, :, :V].sum(0)
    return x if bias is None else x + np.asarray(bias, np.float64)[None, :V]


def log_softmax64(x):
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = x.max(-1, keepdims=True)
        return x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))


def greedy_words(x):
    """Per row of float64 logits: (first index of the maximum, its log-softmax).  The degenerate rows as the kernel comments
    define them: NaNs never win a comparison, so the arg-max runs over the other words and the log-prob is NaN (the sum-exp
    saw the NaN); a row in which no word is above -inf (all NaN, all -inf) gives word 0 and a NaN log-prob."""
    x = np.asarray(x, np.float64)
    words, logp = np.zeros(x.shape[0], np.int64), np.full(x.shape[0], np.nan)
    for b, row in enumerate(x):
        cmp = np.where(np.isnan(row), -np.inf, row)
        if not (cmp > -np.inf).any():
            continue
        words[b] = int(np.argmax(cmp))
        logp[b] = log_softmax64(row[None])[0, words[b]]
    return words, logp


def new_state(B, max_len, n_alive=None, fill=0):
    """the caller-owned state of a rollout before its first step (`fill` in seq / seq_logp: whatever the buffers held)"""
    return dict(seq=np.full((B, max_len), fill, np.int64), seq_logp=np.full((B, max_len), float(fill), np.float64),
                it=np.zeros(B, np.int64), unf=np.ones(B, np.int32), alive=np.zeros(n_alive or max_len + 2, np.int32))


def book_step(words, logp, t, max_len, end, st):
    """editnet_rl.py:529-547 for one timestep, in place: <end> -> 0, the `unfinished` latch (a row that emits word 0 stays
    finished whatever it picks later), seq / seq_logp[:, t] while t < max_len and the loop has not been left
    (alive[t - 1] == 0), alive[t] = rows still unfinished, it = the next input word.  Returns `broken`."""
    it = np.where(np.asarray(words) == end, 0, words).astype(np.int64)
    unf = (it > 0) if t == 0 else ((st["unf"] != 0) & (it > 0))
    it = np.where(unf, it, 0)
    broken = t > 0 and st["alive"][t - 1] == 0
    if t < max_len and not broken:
        st["seq"][:, t] = it
        st["seq_logp"][:, t] = logp
    st["unf"][:] = unf
    st["alive"][t] += int(unf.sum())
    st["it"][:] = it
    return broken


def greedy_step(x, t, max_len, end, st, row_limit=None):
    """one greedy_pick_k launch on float64 logits x (B, V); row_limit: set_decode_row_limits (the word becomes <end> at
    t + 1 >= row_limit[b], the recorded log-prob stays the arg-max's)"""
    words, logp = greedy_words(x)
    if row_limit is not None:
        words = np.where(t + 1 >= np.asarray(row_limit), end, words)
    book_step(words, logp, t, max_len, end, st)
    return words


def relu_embed(E, it):
    return np.maximum(np.asarray(E)[np.asarray(it)], 0)


def sigm(x):
    return 1.0 / (1.0 + np.exp(-x))


def lstm_tail(g0, pre, tab_rows, c_in):
    """the LstmTail cell in float64, operands added in the kernel's order: gate slabs 0, 1, ... (n, B, 4D), then pre (B, 4D) or
    None, then the token-table row (B, 4D); gates i, f, g, o; c' = f c + i g, h' = o tanh c'.  Returns (h', c')."""
    g = np.zeros(np.asarray(tab_rows).shape, np.float64)
    for s in np.asarray(g0, np.float64):
        g = g + s
    if pre is not None:
        g = g + np.asarray(pre, np.float64)
    g = g + np.asarray(tab_rows, np.float64)
    D = g.shape[1] // 4
    i, f, gg, o = (g[:, q * D:(q + 1) * D] for q in range(4))
    c = sigm(f) * np.asarray(c_in, np.float64) + sigm(i) * np.tanh(gg)
    return sigm(o) * np.tanh(c), c


def _bump(flags, key, n=1):
    flags[key] = flags.get(key, 0) + int(n)


def beam_pick(logits, scores, k_left, seqs, best_score, best_seq, best_len, done_score, done_seq, done_len, n_done, cur_len,
              flags, k, V, end, logits2=None):
    """csrc/beam.hip beam_pick_k in numpy, in place (done_* may be None: set_beam_pick_f32).  logits (NI * k, ld >= V).
    One model: float32 throughout; every row's largest logit must stand so far above the others that its log-sum-exp IS that
    logit in float32 (the callers assert 1 + (V - 1) e^-32 == 1), so every candidate value is exact.  With logits2 (the
    ensemble) the log-probabilities log((softmax + softmax2) / 2) are float64 rounded once to float32: values are then
    good to a few ulps only and the caller keeps its candidates apart.  Ties go to the lowest flat index j * V + v.
    flags counts what happened: noop, uncounted_end, tie (two completions of equal score in one pick), zero."""
    NI = scores.shape[0]
    words, rows = np.zeros(NI * k, np.int64), np.zeros(NI * k, np.int32)
    out = seqs.copy()
    for i in range(NI):
        kl = int(k_left[i])
        if kl <= 0:
            rows[i * k:(i + 1) * k] = np.arange(i * k, (i + 1) * k)
            _bump(flags, "noop")
            continue
        vals, valid = np.full(k * V, -np.inf, np.float32), np.zeros(k * V, bool)
        for j in range(k):
            if scores[i, j] == -np.inf:
                continue
            row = logits[i * k + j, :V]
            if logits2 is None:
                lp = (row - row.max()).astype(np.float32)
            else:
                p = np.exp(log_softmax64(row)) + np.exp(log_softmax64(logits2[i * k + j, :V]))
                lp = np.log(p * 0.5).astype(np.float32)
            vals[j * V:(j + 1) * V] = (scores[i, j] + lp).astype(np.float32)
            valid[j * V:(j + 1) * V] = True
        flat_of = np.nonzero(valid)[0]
        best = flat_of[np.argsort(-vals[flat_of], kind="stable")[:k + 64]]       # equal values: ascending flat index
        cand = [(-float(vals[f]), int(f)) for f in best]
        picks = [(np.float32(-nv), flat) for nv, flat in cand[:k]]
        if "picks" in flags:                                             # (the caller wants to look at the candidates)
            flags["picks"].append((i, kl, picks, cand))        # (the best k + 64)
        ends = [(r, v) for r, (v, flat) in enumerate(picks) if r < kl and flat % V == end]
        _bump(flags, "uncounted_end", sum(1 for r, (v, flat) in enumerate(picks) if r >= kl and flat % V == end))
        _bump(flags, "tie", sum(1 for a, b in zip(ends, ends[1:]) if a[1] == b[1]))
        if ends:
            r0 = max(ends, key=lambda e: (e[1], -e[0]))[0]              # first maximum
            if picks[r0][0] > best_score[i]:
                best_score[i], best_len[i] = picks[r0][0], cur_len + 1
                best_seq[i, :cur_len] = seqs[i, picks[r0][1] // V, :cur_len]
                best_seq[i, cur_len] = end
        if n_done is not None:
            for r, v in ends:
                at = int(n_done[i])
                done_score[i, at], done_len[i, at] = v, cur_len + 1
                done_seq[i, at, :cur_len] = seqs[i, picks[r][1] // V, :cur_len]
                done_seq[i, at, cur_len] = end
                n_done[i] += 1
        k_left[i] = kl - len(ends)
        live = [r for r, (v, flat) in enumerate(picks) if r < kl and flat % V != end]
        order = live + [r for r in range(k) if r not in live]
        new_scores = np.full(k, -np.inf, np.float32)
        for slot, r in enumerate(order):
            v, flat = picks[r]
            is_live = r in live
            new_scores[slot] = v if is_live else -np.inf
            words[i * k + slot] = flat % V if is_live else 0
            rows[i * k + slot] = i * k + flat // V
            out[i, slot, :cur_len] = seqs[i, flat // V, :cur_len]
            out[i, slot, cur_len] = flat % V
        scores[i] = new_scores
        _bump(flags, "zero", k_left[i] == 0)
    return out, words, rows
