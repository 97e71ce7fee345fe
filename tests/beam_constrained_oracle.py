"""Test infrastructure: the constrained beam-search pick (include/set_hip.h set_beam_pick_constrained_f32) restated in float64
numpy, and the search around it.  Constraints REMOVE candidates (banned words, <end> before a minimum length, words that would
repeat an n-gram of the slot's own history) and never renormalise; completed hypotheses are ranked by r = x / cur_len^alpha.
tests/test_beam_constrained_cpu.py pins it to oracle/beam_np.beam_loop (neutral constraints) and to hand-written cases of the
n-gram rule; the GPU tests compare the HIP pick and the searches with it."""
import numpy as np

NONE = 0x7fffffff


class Constraints:
    def __init__(self, no_repeat_ngram=0, min_len=0, length_alpha=0.0, banned=()):
        self.no_repeat_ngram, self.min_len, self.length_alpha = int(no_repeat_ngram), int(min_len), float(length_alpha)
        self.banned = tuple(int(b) for b in banned)

    def neutral(self):
        return self.no_repeat_ngram == 0 and self.min_len == 0 and self.length_alpha == 0.0 and not self.banned

    def __repr__(self):
        return "Constraints(n=%d, min_len=%d, alpha=%g, banned=%r)" % (self.no_repeat_ngram, self.min_len, self.length_alpha, self.banned)


NEUTRAL = Constraints()


def log_softmax64(x):
    x = np.asarray(x, np.float64)
    m = x.max(-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        return x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))


def logp64(logits, logits2=None):
    """(rows, V) log-probabilities: log-softmax of one model, or log((softmax + softmax2) / 2)"""
    lp = log_softmax64(logits)
    if logits2 is None:
        return lp
    with np.errstate(divide="ignore"):
        return np.log((np.exp(lp) + np.exp(log_softmax64(logits2))) * 0.5)


def ngram_words(s, n):
    """rule c: the words v that would close an n-gram already in s[1:], s = the slot's tokens with <start> at position 0"""
    L = len(s)
    out = set()
    if n < 1 or L < n:
        return out
    for i in range(1, L - n + 1):
        if list(s[i:i + n - 1]) == list(s[L - n + 1:L]):
            out.add(int(s[i + n - 1]))
    return out


def removed_words(s, c, end):
    """every word v whose candidate (slot with tokens s, v) is removed"""
    out = set(c.banned)
    if len(s) - 1 < c.min_len:
        out.add(int(end))
    return out | ngram_words(s, c.no_repeat_ngram)


def rank_score(x, cur_len, alpha):
    return x if alpha == 0.0 else x / float(cur_len) ** alpha


def new_state(NI, k, Lmax, start, dtype=np.float64):
    st = dict(scores=np.full((NI, k), -np.inf, dtype), k_left=np.full(NI, k, np.int32), seqs=np.full((NI, k, Lmax), start, np.int64),
              best_score=np.full(NI, -np.inf, dtype), best_seq=np.zeros((NI, Lmax), np.int64), best_len=np.zeros(NI, np.int32),
              done_score=np.full((NI, k), -np.inf, dtype), done_seq=np.zeros((NI, k, Lmax), np.int64),
              done_len=np.zeros((NI, k), np.int32), n_done=np.zeros(NI, np.int32))
    st["scores"][:, 0] = 0.0
    return st


def _best(vals, n):
    """the flat indices of the n largest values, equal values in ascending flat index (a stable sort of those that can matter)"""
    n = min(n, len(vals))
    kth = np.partition(vals, len(vals) - n)[len(vals) - n]
    cand = np.nonzero(vals >= kth)[0]
    return cand[np.argsort(-vals[cand], kind="stable")[:n]]


def pick(logits, logits2, st, cur_len, c, k, V, end):
    """One step, in place on st (new_state's arrays, float64 floats).  logits (NI * k, >= V).  -> (seqs_out, words, rows, info);
    info[i] = None for an image that was finished before the step, else a dict:
      top      the k + 1 best surviving (value, flat) pairs (fewer if there are fewer finite ones)
      free_top the best (value, flat) had nothing been removed, `live` = that candidate is one the constraints remove
      counted  how many picks counted, exhausted = the image ended for want of a survivor"""
    NI = st["scores"].shape[0]
    L = cur_len
    lp = logp64(np.asarray(logits)[:, :V], None if logits2 is None else np.asarray(logits2)[:, :V])
    words, rows = np.zeros(NI * k, np.int64), np.zeros(NI * k, np.int32)
    out = st["seqs"].copy()
    info = []
    for i in range(NI):
        kl = int(st["k_left"][i])
        if kl <= 0:
            rows[i * k:(i + 1) * k] = np.arange(i * k, (i + 1) * k)
            info.append(None)
            continue
        vals = np.full(k * V, -np.inf)
        free = np.full(k * V, -np.inf)
        for j in range(k):
            sc = st["scores"][i, j]
            if sc == -np.inf:
                continue
            x = sc + lp[i * k + j]
            free[j * V:(j + 1) * V] = x
            x = x.copy()
            gone = [w for w in removed_words(st["seqs"][i, j, :L], c, end) if 0 <= w < V]
            x[gone] = -np.inf
            vals[j * V:(j + 1) * V] = x
        vals[np.isnan(vals)] = -np.inf
        free[np.isnan(free)] = -np.inf
        order = _best(vals, k + 1)
        top = [(float(vals[f]), int(f)) for f in order if vals[f] > -np.inf]
        f0 = int(_best(free, 1)[0])
        inf_i = dict(top=top, free_top=(float(free[f0]), f0), live=bool(free[f0] > -np.inf and vals[f0] == -np.inf),
                     counted=0, exhausted=not top)
        info.append(inf_i)
        picks = [(top[r][0], top[r][1]) if r < len(top) else (-np.inf, NONE) for r in range(k)]
        if not top:                                                       # exhausted: the image ends here
            st["k_left"][i] = 0
            st["scores"][i] = -np.inf
            rows[i * k:(i + 1) * k] = np.arange(i * k, (i + 1) * k)
            continue
        ok = [flat != NONE and r < kl for r, (v, flat) in enumerate(picks)]
        inf_i["counted"] = sum(ok)
        ends = [r for r, (v, flat) in enumerate(picks) if ok[r] and flat % V == end]
        rs = {r: rank_score(picks[r][0], L, c.length_alpha) for r in ends}
        if ends:
            r0 = max(ends, key=lambda r: (rs[r], -r))                    # first maximum
            if rs[r0] > st["best_score"][i]:
                st["best_score"][i], st["best_len"][i] = rs[r0], L + 1
                st["best_seq"][i, :L] = st["seqs"][i, picks[r0][1] // V, :L]
                st["best_seq"][i, L] = end
        for r in ends:
            at = int(st["n_done"][i])
            if at >= k:
                continue
            st["done_score"][i, at], st["done_len"][i, at] = rs[r], L + 1
            st["done_seq"][i, at, :L] = st["seqs"][i, picks[r][1] // V, :L]
            st["done_seq"][i, at, L] = end
            st["n_done"][i] += 1
        st["k_left"][i] = kl - len(ends)
        live = [r for r in range(k) if ok[r] and r not in ends]
        new_scores = np.full(k, -np.inf)
        for slot, r in enumerate(live + [r for r in range(k) if r not in live]):
            v, flat = picks[r]
            parent, word = (flat // V, flat % V) if flat != NONE else (0, 0)
            new_scores[slot] = v if r in live else -np.inf
            words[i * k + slot] = word if r in live else 0
            rows[i * k + slot] = i * k + parent
            out[i, slot, :L] = st["seqs"][i, parent, :L]
            out[i, slot, L] = word
        st["scores"][i] = new_scores
    return out, words, rows, info


def min_gap(info):
    """the smallest difference between adjacent entries of the top k + 1 over the images of one step"""
    g = np.inf
    for inf_i in info:
        if inf_i:
            v = [x for x, _ in inf_i["top"]]
            g = min([g] + [a - b for a, b in zip(v, v[1:])])
    return g


def rank_gap(st):
    """the smallest difference between the rank scores of two completed hypotheses of one image"""
    g = np.inf
    for i in range(st["scores"].shape[0]):
        v = sorted(st["done_score"][i, :int(st["n_done"][i])], reverse=True)
        g = min([g] + [a - b for a, b in zip(v, v[1:])])
    return g


def search(step, reindex, NI, k, V, start, end, c, max_steps):
    """evaluate._fused_beam on the oracle's pick.  step(words (NI * k)) -> list of one or two (NI * k, V) logits;
    reindex(rows (NI * k)) re-indexes the models' state.  -> (answers, nbest, steps): answers[i] = (tokens, score) — the best
    completed hypothesis by rank score, (seqs[0][:18], nan) at the step limit, ([start], nan) when the image ran out of candidates
    before anything completed; nbest[i] = every completed (tokens, r) sorted by r, equal r in completion order; steps = the info of
    every pick."""
    Lmax = max_steps + 2
    st = new_state(NI, k, Lmax, start)
    words = np.full(NI * k, start, np.int64)
    steps = []
    for cur in range(1, max_steps + 2):
        lg = step(words)
        out, words, rows, info = pick(lg[0], lg[1] if len(lg) > 1 else None, st, cur, c, k, V, end)
        st["seqs"] = out
        reindex(rows)
        steps.append(info)
        if int(st["k_left"].max()) == 0:
            break
    answers, nbest = [], []
    for i in range(NI):
        if st["k_left"][i] > 0:
            answers.append((st["seqs"][i, 0, :18].tolist(), float("nan")))
        elif st["best_len"][i] == 0:
            answers.append(([start], float("nan")))
        else:
            answers.append((st["best_seq"][i, :st["best_len"][i]].tolist(), float(st["best_score"][i])))
        done = [(st["done_seq"][i, j, :st["done_len"][i, j]].tolist(), float(st["done_score"][i, j])) for j in range(int(st["n_done"][i]))]
        nbest.append(sorted(done, key=lambda e: -e[1]))
    return answers, nbest, steps
