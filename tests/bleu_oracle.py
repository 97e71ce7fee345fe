"""Float64 restatement of coco-caption's BleuScorer (n = 4, option "closest"), written from the metric's definition with
collections.Counter over tuples and independent of show_edit_tell_amd/bleu.py: the yardstick of tests/test_bleu_cpu.py and
tests/test_hip_bleu_device.py.

    guess[k]   = max(0, len(h) - k + 1)
    correct[k] = sum over distinct k-grams g of h: min(count_h(g), max_r count_r(g))
    reflen     = the len(r) minimising (|len(r) - len(h)|, len(r))
    b *= (correct[k] + 1e-15) / (guess[k] + 1e-9); bleu[k] = b ** (1/k); ratio = (testlen + 1e-15) / (reflen + 1e-9);
    ratio < 1: bleu[k] *= exp(1 - 1/ratio)
"""
import math
from collections import Counter


def ngrams(s, k):
    return Counter(tuple(s[i:i + k]) for i in range(0, len(s) - k + 1))


def stats(h, R):
    """[correct_1..4, guess_1..4, testlen, reflen] of hypothesis h (list) against the references R (list of lists)"""
    correct, guess = [], []
    for k in (1, 2, 3, 4):
        hyp = ngrams(h, k)
        refs = [ngrams(r, k) for r in R]
        correct.append(sum(min(c, max([rc[g] for rc in refs], default=0)) for g, c in hyp.items()))
        guess.append(max(0, len(h) - k + 1))
    reflen = sorted((abs(len(r) - len(h)), len(r)) for r in R)[0][1] if R else 0
    return correct + guess + [len(h), reflen]


def score(st):
    """bleu[1..4] from ten statistics (one sentence's, or sums over a corpus)"""
    tiny, small = 1e-15, 1e-9
    correct, guess, testlen, reflen = st[0:4], st[4:8], st[8], st[9]
    bleu, b = [], 1.0
    for k in (1, 2, 3, 4):
        b *= (float(correct[k - 1]) + tiny) / (float(guess[k - 1]) + small)
        bleu.append(b ** (1.0 / k))
    ratio = (float(testlen) + tiny) / (float(reflen) + small)
    if ratio < 1:
        bleu = [x * math.exp(1 - 1 / ratio) for x in bleu]
    return bleu


def sentence(h, R):
    return score(stats(h, R))


def corpus(pairs):
    """pairs: iterable of (h, R) -> the four corpus scores (statistics summed, then scored)"""
    tot = [0] * 10
    for h, R in pairs:
        tot = [a + b for a, b in zip(tot, stats(h, R))]
    return score(tot)


def cut_after_zero(row):
    """the decoder's rule: a row ends after its first 0, the 0 stays; no 0: the whole row"""
    row = [int(w) for w in row]
    return row[:row.index(0) + 1] if 0 in row else row
