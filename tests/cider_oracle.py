"""float64 oracle of cocoEval's `CIDEr` on id lists, independent of show_edit_tell_amd.ciderd (its own gram counting, its own
table), for tests/test_cider_corpus_cpu.py and tests/test_hip_cider_corpus.py:

    df(g)       = the number of reference SETS one of whose references holds the gram g (once per set)
    w(s, g)     = count of g in s * (log N - log max(1, df(g))),   N = the number of sets
    sim_k(h, r) = sum over the order-k grams g of h that r holds: min(w(h, g), w(r, g)) * w(r, g) / (|w_k(h)| |w_k(r)|)
                  * exp(-(l_h - l_r)^2 / (2 sigma^2)),   l = the number of bigrams (0 with n = 1), the division only where both
                  norms are non-zero
    score(h)    = 10 / (n max(1, |R|)) * sum_k sum_{r in R} sim_k(h, r);   the corpus value is the mean of the scores

Also the fixture the two test files share: world(), the captions and reference sets of tests/test_hip_rouge_validation.py::_world,
rebuilt here from its recipe."""
import math

import numpy as np


def grams(seq, n=4):
    """{gram tuple: count} of the orders 1 .. n"""
    seq = [int(w) for w in seq]
    out = {}
    for k in range(1, n + 1):
        for i in range(len(seq) - k + 1):
            g = tuple(seq[i:i + k])
            out[g] = out.get(g, 0) + 1
    return out


def document_frequency(sets, n=4, leave_out=()):
    """{gram: number of sets that hold it}; leave_out: (set index, reference index) pairs whose grams are not counted"""
    df = {}
    for s, refs in enumerate(sets):
        seen = set()
        for j, r in enumerate(refs):
            if (s, j) not in leave_out:
                seen.update(grams(r, n))
        for g in seen:
            df[g] = df.get(g, 0) + 1
    return df


def _vector(seq, df, log_n, n):
    vec = [dict() for _ in range(n)]
    for g, tf in grams(seq, n).items():
        vec[len(g) - 1][g] = tf * (log_n - math.log(max(1.0, float(df.get(g, 0)))))
    norm = [math.sqrt(math.fsum(w * w for w in v.values())) for v in vec]
    bigrams = max(0, len(seq) - 1) if n >= 2 else 0
    return vec, norm, bigrams


def sentence(hyp, refs, df, n_docs, n=4, sigma=6.0):
    log_n = math.log(float(n_docs))
    vh, nh, lh = _vector(hyp, df, log_n, n)
    terms = []
    for r in refs:
        vr, nr, lr = _vector(r, df, log_n, n)
        pen = math.exp(-float(lh - lr) ** 2 / (2.0 * sigma * sigma))
        for k in range(n):
            s = math.fsum(min(w, vr[k][g]) * vr[k][g] for g, w in vh[k].items() if g in vr[k])
            if nh[k] != 0.0 and nr[k] != 0.0:
                s /= nh[k] * nr[k]
            terms.append(s * pen)
    return math.fsum(terms) / n / max(1, len(refs)) * 10.0


def corpus(hyps, hyp_set, sets, n=4, sigma=6.0, df=None):
    """(mean, [score of every hypothesis]); df and N from ALL of `sets` (or the df given, N = len(sets))"""
    df = document_frequency(sets, n) if df is None else df
    scores = [sentence(h, sets[s], df, len(sets), n, sigma) for h, s in zip(hyps, hyp_set)]
    return (math.fsum(scores) / len(scores) if scores else 0.0), scores


V = 60


def world():
    """tests/test_hip_rouge_validation.py::_world: 37 captions of 0..18 words over w1..w40, each with its own 1..5 references
    (near-copies and random ones, <end> = 0 last), in the decoder's format (0 = <end>, junk behind it) and as token lists in the
    vocabulary's ids; list 3 never reached <end>, row 5 of the tensor is full (no 0)"""
    from show_edit_tell_amd import synth
    wm = synth.word_map(V)
    start, end, pad = wm["<start>"], wm["<end>"], wm["<pad>"]
    rng = np.random.default_rng(21)
    N, L = 37, 19
    words, gt = [], []
    for i in range(N):
        n = L if i == 5 else int(rng.integers(0, 19))
        c = [int(x) for x in rng.integers(1, 41, n)]
        words.append(c)
        refs = []
        for j in range(1 + i % 5):
            if j % 2 == 0 and n > 1:
                r = list(c)
                r[int(rng.integers(0, n))] = int(rng.integers(1, 41))
                r = r[:max(1, n - j)]
            else:
                r = [int(x) for x in rng.integers(1, 41, int(rng.integers(1, 15)))]
            refs.append(r + [0])
        gt.append(refs)
    T = np.zeros((N, L), dtype=np.int64)
    for i, c in enumerate(words):
        T[i, :len(c)] = c
        T[i, len(c) + 1:] = rng.integers(0, 41, max(0, L - len(c) - 1))       # behind the first 0: junk
    assert 0 not in T[5] and any(len(c) == 0 for c in words)
    lists = [[start] + c + ([] if i == 3 else [end]) + [pad] * (i % 3) for i, c in enumerate(words)]
    assert len(words[3]) > 0
    return dict(wm=wm, words=words, gt=gt, T=T, lists=lists, N=N)


def world_sides(w, count_end, lists=False):
    """(hypotheses, reference sets) of the world as the metric sees them; count_end: the 0 is a token on both sides — for a
    caption that holds one (list 3 and row 5 do not)"""
    hyps = []
    for i, c in enumerate(w["words"]):
        ended = (i != 3) if lists else (i != 5)
        hyps.append(c + [0] if (count_end and ended) else list(c))
    sets = [[r if count_end else r[:-1] for r in refs] for refs in w["gt"]]
    return hyps, sets
