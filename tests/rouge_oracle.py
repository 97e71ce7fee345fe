"""Float64 restatement of coco-caption's Rouge (ROUGE-L, beta = 1.2) on token lists, written from the metric's definition with
the textbook (m + 1) x (n + 1) table and independent of show_edit_tell_amd/rouge.py: the yardstick of tests/test_rouge_cpu.py
and the tests/test_hip_rouge_*.py files.

    lcs(h, r)  = the length of the longest common subsequence
    lcs_p      = max_r lcs(h, r)
    (lcs_r, len_r) = the reference of the largest recall lcs / len(r): fractions compared exactly, of equal ones the first,
                 references of no tokens skipped unless all are empty: (0, 0)
    P = lcs_p / len(h), Rc = lcs_r / len_r;  score = (1 + beta^2) P Rc / (Rc + beta^2 P) when both are non-zero, else 0
    corpus = the mean of the sentence scores
"""
from fractions import Fraction

BETA = 1.2


def lcs(a, b):
    """textbook dynamic programme: T[i][j] = LCS of a[:i] and b[:j]"""
    m, n = len(a), len(b)
    T = [[0] * (n + 1) for _ in range(m + 1)]
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            T[i][j] = T[i - 1][j - 1] + 1 if a[i - 1] == b[j - 1] else max(T[i - 1][j], T[i][j - 1])
    return T[m][n]


def stats(h, R):
    """[lcs_p, len_h, lcs_r, len_r] of hypothesis h (list) against the references R (list of lists)"""
    ls = [lcs(h, r) for r in R]
    lcs_p = max(ls, default=0)
    best = None                                                    # (recall, lcs, len) of the first largest recall
    for l, r in zip(ls, R):
        if len(r) == 0:
            continue
        rec = Fraction(l, len(r))
        if best is None or rec > best[0]:
            best = (rec, l, len(r))
    return [lcs_p, len(h), best[1], best[2]] if best is not None else [lcs_p, len(h), 0, 0]


def score(st, beta=BETA):
    lcs_p, len_h, lcs_r, len_r = (int(x) for x in st)
    if len_h == 0 or len_r == 0 or lcs_p == 0 or lcs_r == 0:
        return 0.0
    b2 = beta * beta
    P = lcs_p / len_h
    Rc = lcs_r / len_r
    return (1.0 + b2) * P * Rc / (Rc + b2 * P)


def sentence(h, R, beta=BETA):
    return score(stats(h, R), beta)


def corpus(pairs, beta=BETA):
    """pairs: iterable of (h, R) -> the mean of the sentence scores"""
    s = [sentence(h, R, beta) for h, R in pairs]
    return sum(s) / len(s) if s else 0.0


def cut_after_zero(row):
    """the decoder's rule: a row ends after its first 0, the 0 stays; no 0: the whole row"""
    row = [int(w) for w in row]
    return row[:row.index(0) + 1] if 0 in row else row


def grid(seed=11):
    """The fixed-seed grid of both test files: lengths {0, 1, 2, 7, 63, 64} on both sides, alphabets of 1, 2 and 30 symbols,
    sets of 1 and 5 references.  Returns a list of (h, R) with ids >= 1.  In a set of 5 the first reference has the grid
    length, the others rotate through the lengths (so empty references sit beside others, and recalls tie in small alphabets)."""
    import random
    rng = random.Random(seed)
    lengths = (0, 1, 2, 7, 63, 64)
    out = []
    for A in (1, 2, 30):
        words = lambda n: [rng.randint(1, A) for _ in range(n)]
        for lh in lengths:
            for a, lr in enumerate(lengths):
                h = words(lh)
                out.append((h, [words(lr)]))
                R = [words(lr)] + [words(lengths[(a + k) % len(lengths)]) for k in range(1, 5)]
                if A == 30 and lh > 2:                             # large alphabet: make something match, a mutated copy
                    c = list(h)
                    c[rng.randrange(len(c))] = rng.randint(1, A)
                    R[2] = c[:lengths[(a + 2) % len(lengths)]] or R[2]
                out.append((h, R))
    return out
